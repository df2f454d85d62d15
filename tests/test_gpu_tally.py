"""GPU: the tally (libfsm_amd/csrc/tally.hip: tally_spans and the fronts): matches and lines per rule and per group.

Every table is compared with tests/tally_ref.py -- np.bincount over col(id) per group, distinct (input, col) pairs for lines --
never with anything that came from the device.  The first half feeds synthetic off / id / group_off arrays to
fsm_hip_tally_ids_device; the second half runs the real objects over tests/line_inputs.py's keyword lines (five rules, line 8 =
300 times d) and s15_start as `ends` (NO_ID alone, empty matches), whose ids and offsets are line_inputs.reference's.
Every device table is two rows too long and pre-filled: nothing behind G * C may change, and without FSM_HIP_TALLY_ADD nothing of
the pattern may survive inside."""
import ctypes as C
import errno
import functools
import os
import subprocess

import numpy as np
import pytest

import matches_ref
import span_ref
import tally_ref
import tokens_ref
from line_inputs import FILL, KEYWORDS, SIZES, auto_of, device_u64, device_u8, ends_image, inputs_of, judged, lead_packed, reference, starts_image, state_ids
from matches_ref import DROP_EMPTY
from tally_ref import NO_ID, NO_MATCH
from tokens_ref import SKIP_BAD

pytestmark = pytest.mark.gpu

NL = 0x0A
LONG = 70000


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()   # raises if the HIP extension is missing: no silent fallback
    return libfsm_amd


def device_u32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).cuda()


class Table:
    """a device table of G x C entries, two rows (at least two entries) too long, pre-filled with FILL or, inside, with `pre`"""

    def __init__(self, G, Cn, pre=None):
        self.G, self.C = G, Cn
        host = np.full(G * Cn + 2 * Cn + 2, FILL, np.uint64)
        if pre is not None:
            host[:G * Cn] = np.asarray(pre, np.uint64).ravel()
        self.dev = device_u64(host)
        self.ptr = self.dev.data_ptr()

    def read(self, what=None):
        """the G x C entries; nothing behind them has changed"""
        got = self.dev.cpu().numpy().view(np.uint64)
        assert (got[self.G * self.C:] == FILL).all(), (what, "a store behind G * C")
        return got[:self.G * self.C].reshape(self.G, self.C)


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, "first (group, column)", bad[:5].tolist(), [int(got[tuple(b)]) for b in bad[:5]], [int(want[tuple(b)]) for b in bad[:5]])


def run_ids(hip, off, ids, nrules, goff=None, which=(True, True), flags=0, pre=(None, None), m=None, total=None, ngroups=None):
    """fsm_hip_tally_ids_device over device copies of the arrays -> [count, lines] as read back (None where not asked for)"""
    import torch
    off, ids = np.asarray(off, np.uint64), np.asarray(ids, np.uint32)
    d_off = device_u64(off)
    d_id = device_u32(ids if len(ids) else np.zeros(1, np.uint32))
    d_goff = device_u64(goff) if goff is not None else None
    G = (len(goff) - 1 if goff is not None else 1) if ngroups is None else ngroups
    tabs = [Table(G, nrules + 1, p) if w else None for w, p in zip(which, pre)]
    hip.tally_ids_device(d_off.data_ptr(), d_id.data_ptr(), len(off) - 1 if m is None else m, len(ids) if total is None else total,
                         d_goff.data_ptr() if d_goff is not None else 0, G if goff is not None else 0, nrules,
                         tabs[0].ptr if tabs[0] else 0, tabs[1].ptr if tabs[1] else 0, flags)
    torch.cuda.synchronize()
    return [t.read((nrules, G)) if t else None for t in tabs]


def check_ids(hip, off, ids, nrules, goff=None, what=None, forms=((True, True),)):
    """the device's tables against the judge's, in every form of `forms`: (count, lines) asked for or not"""
    want = tally_ref.tally(off, ids, nrules, goff)
    for which in forms:
        got = run_ids(hip, off, ids, nrules, goff, which)
        for name, g, w, asked in zip(("count", "lines"), got, want, which):
            assert (g is not None) == asked
            if asked:
                same(g, w, (what, name, which))
    return want


ALL_FORMS = ((True, True), (True, False), (False, True))


def offsets_of(counts, first=0):
    return np.concatenate([[first], first + np.cumsum(counts)]).astype(np.uint64)


def special_ids(rng, total, nrules):
    """random ids below nrules + 2 with nrules - 1, nrules, NO_ID and NO_MATCH planted"""
    ids = rng.randint(0, nrules + 2, total).astype(np.uint32)
    r = rng.randint(0, 16, total)
    ids[r == 0] = NO_MATCH
    ids[r == 1] = NO_ID
    ids[r == 2] = max(nrules, 1) - 1
    ids[r == 3] = nrules
    return ids


def long_batch(rng, kind, nrules):
    """an input of 70 000 entries in mid-batch among inputs of 0-3: (off, ids, the long input's index)"""
    counts = rng.randint(0, 4, 201)
    at = 100
    counts[at] = LONG
    off = offsets_of(counts)
    total = int(off[-1])
    ids = special_ids(rng, total, nrules)
    a, b = int(off[at]), int(off[at + 1])
    if kind == "one column":
        ids[a:b] = min(2, nrules)
    elif kind == "cycling":
        ids[a:b] = np.arange(b - a) % (nrules + 1)                           # (nrules itself: the other column)
    return off, ids, at


# ---- the synthetic half: fsm_hip_tally_ids_device --------------------------------------------------------------------------------

def test_every_size_and_every_count_per_input(hip):
    """m in SIZES; per input 0, 1, 2, window - 1, window, window + 1, 3 * window + 5 entries in one batch; ids that include
    nrules - 1, nrules, NO_ID and NO_MATCH; count alone, lines alone and both"""
    W = hip.tally_window()
    kinds = np.array([0, 1, 2, W - 1, W, W + 1, 3 * W + 5])
    rng = np.random.RandomState(3)
    for m in SIZES:
        counts = kinds[(np.arange(m) * 5 + 3) % 7] if m >= 7 else kinds[[6]][:m]
        if m >= 7:
            assert set(counts.tolist()) == set(kinds.tolist())
        off = offsets_of(counts, first=2)                                   # two ids in front that no input owns
        ids = special_ids(rng, int(off[-1]) + 3, 5)                         # ... and three behind
        want = check_ids(hip, off, ids, 5, None, ("sizes", m), ALL_FORMS)
        assert int(want[0].sum()) == int(counts.sum()) and (m < 64 or (want[0] > 0).all())
        goff = np.unique(np.concatenate([[0, m], rng.randint(0, m + 1, 6)])).astype(np.uint64)
        check_ids(hip, off, ids, 5, goff, ("sizes, groups", m))
    assert set(np.unique(ids).tolist()) >= {4, 5, NO_ID, NO_MATCH}


@pytest.mark.parametrize("kind", ["one column", "cycling", "random"])
def test_one_input_of_70000_entries(hip, kind):
    """... in mid-batch, among inputs of 0-3 entries: the windows of one workgroup, a backward look that ends at its first step
    (one column), after C steps (cycling), or runs through the window (random over many columns); a group boundary directly
    before and directly behind the long input"""
    rng = np.random.RandomState(len(kind))
    for nrules in (5, 700) if kind == "random" else (5,):
        off, ids, at = long_batch(rng, kind, nrules)
        m = len(off) - 1
        want = check_ids(hip, off, ids, nrules, None, (kind, nrules, "one group"), ALL_FORMS)
        assert int(want[0].sum()) == int(off[-1]) > LONG
        if kind == "one column":
            assert int(want[0][0, 2]) >= LONG and int(want[1][0, 2]) < 201
        for goff in ([0, at, at + 1, m], [0, at, m], [0, at + 1, m], [at, at + 1], [3, at - 1, at, at, at + 1, at + 1, at + 2, m - 2]):
            w = check_ids(hip, off, ids, nrules, np.array(goff, np.uint64), (kind, nrules, goff))
            g = goff.index(at) if at in goff else None
            if goff == [at, at + 1]:
                assert int(w[0].sum()) == LONG
            elif g is not None and goff[g + 1] == at + 1:
                assert int(w[0][g].sum()) == LONG


def test_columns_on_both_sides_of_the_caps(hip):
    """nrules 0, 1, 5, around fsm_hip_tally_lds_columns() and at fsm_hip_tally_max_line_columns() - 1; one column above it is ENOTSUP
    with lines and works with lines == NULL"""
    L, M = hip.tally_lds_columns(), hip.tally_max_line_columns()
    W = hip.tally_window()
    rng = np.random.RandomState(8)
    counts = rng.choice([0, 1, 2, 5, W + 3, 2 * W], 300)
    off = offsets_of(counts)
    total = int(off[-1])
    for nrules in (0, 1, 5, L - 2, L - 1, L, L + 1, M - 1):
        ids = special_ids(rng, total, nrules)
        for G, goff in ((1, None), (2, np.array([0, 150, 300], np.uint64))):
            want = check_ids(hip, off, ids, nrules, goff, ("columns", nrules, G), ALL_FORMS if G == 1 else ((True, True),))
            assert want[0].shape == (G, nrules + 1) and int(want[0][:, nrules].sum()) > 0
    ids = special_ids(rng, total, M)
    with pytest.raises(OSError) as ei:
        run_ids(hip, off, ids, M, None, (True, True))
    assert ei.value.errno == errno.ENOTSUP
    with pytest.raises(OSError) as ei:
        run_ids(hip, off, ids, M, None, (False, True))
    assert ei.value.errno == errno.ENOTSUP
    got = run_ids(hip, off, ids, M, None, (True, False))
    same(got[0], tally_ref.tally(off, ids, M)[0], "count alone above the cap of lines")


def test_groups(hip):
    """one group; a boundary at every input of the first 70; runs of 1, 2 and 300 empty groups; group_off[0] > 0 and group_off[G]
    < m; boundaries on, one below and one above a multiple of fsm_hip_tally_span_inputs()"""
    S, W = hip.tally_span_inputs(), hip.tally_window()
    rng = np.random.RandomState(4)
    m = 1500
    counts = rng.choice([0, 0, 1, 2, 3, 7, W + 1], m, p=[.2, .2, .2, .15, .15, .08, .02])
    off = offsets_of(counts)
    ids = special_ids(rng, int(off[-1]), 5)
    edges = [k * S + d for k in (1, 2, 5, 11) for d in (-1, 0, 1)]
    every = list(range(71))
    cases = {
        "one group": [0, m],
        "every input of the first 70": every + [m],
        "empty runs": [0, 10, 10, 20, 20, 20, 30] + [40] * 301 + [41, m],
        "inside": [7, 100, 1400],
        "inside, one input": [777, 778],
        "span edges": sorted([0, m] + edges),
        "all": sorted([5] + every[6:] + edges + [300] * 301 + [900, 900, 901, 901, 901, 1499]),
        "nothing": [m, m],
        "empty at both ends": [0, 0, m, m],
    }
    for what, goff in cases.items():
        goff = np.array(goff, np.uint64)
        want = check_ids(hip, off, ids, 5, goff, what, ALL_FORMS if what in ("all", "inside") else ((True, True),))
        empty = np.flatnonzero(np.diff(goff.astype(np.int64)) == 0)
        assert (want[0][empty] == 0).all()
        if what == "inside":
            assert int(want[0].sum()) == int(off[1400] - off[7]) < int(off[-1])
        if what == "nothing":
            assert int(want[0].sum()) == 0
    # more granules than workgroups: a workgroup takes several, and 1 000 groups fall anywhere
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m = S * cus * 3 * 2 + 17
    counts = rng.choice([0, 1, 2, 3], m)
    off = offsets_of(counts)
    ids = special_ids(rng, int(off[-1]), 5)
    goff = np.unique(np.concatenate([[0, m], rng.randint(0, m + 1, 1000)])).astype(np.uint64)
    check_ids(hip, off, ids, 5, goff, "many granules, 1 000 groups")
    check_ids(hip, off, ids, 5, None, "many granules, one group", ALL_FORMS)


def test_add_twice_onto_a_pattern(hip):
    """FSM_HIP_TALLY_ADD onto pre-filled tables, twice in a row; then without it: nothing of the pattern survives"""
    import torch
    rng = np.random.RandomState(6)
    counts = rng.choice([0, 1, 4, 300], 400)
    off = offsets_of(counts)
    ids = special_ids(rng, int(off[-1]), 5)
    goff = np.array([0, 100, 100, 350, 400], np.uint64)
    want = tally_ref.tally(off, ids, 5, goff)
    G, Cn = want[0].shape
    pattern = [(np.arange(G * Cn, dtype=np.uint64) * np.uint64(k) + np.uint64(11)).reshape(G, Cn) for k in (3, 1000003)]
    pattern[1][0, 0] = np.uint64(2 ** 64 - 1)                               # (the add wraps as u64 does)
    d_off, d_id, d_goff = device_u64(off), device_u32(ids), device_u64(goff)
    tabs = [Table(G, Cn, p) for p in pattern]
    args = (d_off.data_ptr(), d_id.data_ptr(), len(off) - 1, len(ids), d_goff.data_ptr(), G, 5, tabs[0].ptr, tabs[1].ptr)
    for k in (1, 2):
        hip.tally_ids_device(*args, flags=hip.TALLY_ADD)
        torch.cuda.synchronize()
        for t, p, w, name in zip(tabs, pattern, want, ("count", "lines")):
            same(t.read(), p + np.uint64(k) * w, ("add", k, name))
    hip.tally_ids_device(*args)
    torch.cuda.synchronize()
    for t, w, name in zip(tabs, want, ("count", "lines")):
        same(t.read(), w, ("cleared", name))
    # ... and count alone
    got = run_ids(hip, off, ids, 5, goff, (True, False), hip.TALLY_ADD, (pattern[0], None))
    same(got[0], pattern[0] + want[0], "count alone, added")


def test_broken_arrays_leave_the_device_usable(hip):
    """an off with entries above total is defined: they are the total.  An off or a group_off that decreases gives counts nobody
    asserts; the call returns, nothing behind the tables changes (run_ids looks), and the next correct call is right"""
    rng = np.random.RandomState(12)
    counts = rng.choice([0, 1, 3, 260], 300)
    off = offsets_of(counts)
    total = int(off[-1])
    ids = special_ids(rng, total, 5)
    goff = np.array([0, 50, 120, 300], np.uint64)
    short = total // 2
    check_ids(hip, off, ids[:short], 5, goff, "off above total", ALL_FORMS)
    huge = off.copy()
    huge[200:] = np.uint64(2 ** 64 - 1)
    check_ids(hip, huge, ids, 5, goff, "off at 2^64 - 1")
    bad_off = off.copy()
    bad_off[rng.randint(0, 301, 60)] = rng.randint(0, total + 1000, 60).astype(np.uint64)
    bad_off[17] = np.uint64(2 ** 63)
    bad_goff = np.array([200, 50, 2 ** 64 - 1, 10, 300, 0], np.uint64)
    for o, g in ((bad_off, goff), (off, bad_goff), (bad_off, bad_goff), (off[::-1].copy(), bad_goff)):
        for which in ALL_FORMS:
            run_ids(hip, o, ids, 5, g, which)
        run_ids(hip, o, ids, hip.tally_lds_columns() + 5, g)
    check_ids(hip, off, ids, 5, goff, "the next correct call", ALL_FORMS)


def test_no_entries_and_no_inputs(hip):
    """total == 0 and m == 0: the tables are cleared, unless they are added to, and nothing else is launched"""
    off0 = np.zeros(6, np.uint64)
    goff = np.array([0, 2, 5], np.uint64)
    pre = np.arange(12, dtype=np.uint64).reshape(2, 6) + np.uint64(5)
    for off, ids, m, total in ((off0, [], None, None), (np.zeros(1, np.uint64), [], None, None), (np.zeros(1, np.uint64), [1, 2, 3], 0, 3),
                               (np.array([0, 1, 2, 3, 4, 5], np.uint64), [0, 1, 2, 3, 4], None, 0)):
        g = goff if m is None and len(off) == 6 else np.array([0, 0, 0], np.uint64)
        for which in ALL_FORMS:
            got = run_ids(hip, off, ids, 5, g, which, m=m, total=total)
            assert all(t is None or (t == 0).all() for t in got)
            got = run_ids(hip, off, ids, 5, g, which, hip.TALLY_ADD, (pre, pre), m=m, total=total)
            assert all(t is None or np.array_equal(t, pre) for t in got)
        got = run_ids(hip, off, ids, 0, None, m=m, total=total)
        assert got[0].tolist() == [[0]] and got[1].tolist() == [[0]]


def test_refusals_with_a_device(hip):
    """EINVAL, EOVERFLOW and ENOTSUP before any launch, and the next call answers"""
    lib = hip.load_library()
    off = offsets_of([2, 0, 1])
    ids = np.array([0, 1, 7], np.uint32)
    d_off, d_id, d_goff = device_u64(off), device_u32(ids), device_u64(np.array([0, 3], np.uint64))
    t = Table(1, 3)
    o, i, g, p = d_off.data_ptr(), d_id.data_ptr(), d_goff.data_ptr(), t.ptr
    M = hip.tally_max_line_columns()
    for args, want in (((o, i, 3, 3, None, 0, 2, 0, None, None, None), errno.EINVAL),          # both tables NULL
                       ((o, i, 3, 3, None, 0, 2, 2, p, None, None), errno.EINVAL),             # an unknown flag bit
                       ((o, i, 3, 3, None, 0, 2, 0x80000001, p, None, None), errno.EINVAL),
                       ((o, i, 3, 3, g, 0, 2, 0, p, None, None), errno.EINVAL),                # ngroups == 0 with group_off
                       ((None, i, 3, 3, None, 0, 2, 0, p, None, None), errno.EINVAL),
                       ((o, None, 3, 3, None, 0, 2, 0, p, None, None), errno.EINVAL),
                       ((o, i, 3, 3, g, 2 ** 61, 7, 0, p, None, None), errno.EOVERFLOW),       # G * C * 8 = 2^67
                       ((o, i, 3, 3, g, 1, 2 ** 64 - 1, 0, p, None, None), errno.EOVERFLOW),   # C = 2^64
                       ((o, i, 3, 3, None, 0, M, 0, None, p, None), errno.ENOTSUP),
                       ((o, i, 3, 3, g, 1, M, 0, p, p, None), errno.ENOTSUP)):
        C.set_errno(0)
        assert lib.fsm_hip_tally_ids_device(*args) == -1 and C.get_errno() == want, args
    assert (t.read() == FILL).all()
    pd, td = starts_image("kw_starts"), ends_image("kw_ends")
    rows, lens = inputs_of("kw_ends")
    data, poff = lead_packed(rows[:64], lens[:64])
    mt = hip.HipMatches.run(pd, td, data, poff)
    tk = td.tokens(data, poff)
    out = np.zeros(12, np.uint64)
    hp = out.ctypes.data_as(C.c_void_p)
    for obj, host, dev in ((mt, lib.fsm_hip_matches_tally, lib.fsm_hip_matches_tally_device), (tk, lib.fsm_hip_tokens_tally, lib.fsm_hip_tokens_tally_device)):
        h = C.c_void_p(obj.handle)
        for goff in ([0, 65], [0, 30, 20, 64], [5, 4]):                                       # exceeds m; decreases
            ga = np.array(goff, np.uint64)
            C.set_errno(0)
            assert host(h, ga.ctypes.data_as(C.c_void_p), len(goff) - 1, 5, 0, hp, None) == -1 and C.get_errno() == errno.EINVAL, goff
        for args in ((None, None, 0, 5, 0, hp, None), (h, None, 0, 5, 0, None, None), (h, None, 0, 5, 4, hp, None), (h, hp, 0, 5, 0, hp, None)):
            C.set_errno(0)
            assert host(*args) == -1 and C.get_errno() == errno.EINVAL, args
        for args in ((None, None, 0, 5, 0, p, None, None), (h, None, 0, 5, 0, None, None, None), (h, g, 0, 5, 0, p, None, None)):
            C.set_errno(0)
            assert dev(*args) == -1 and C.get_errno() == errno.EINVAL, args
        C.set_errno(0)
        assert host(h, None, 0, M, 0, hp, hp) == -1 and C.get_errno() == errno.ENOTSUP
    assert (out == 0).all()
    res = matches_ref.head(reference("kw_starts", "kw_ends"), 64)
    want = tally_ref.tally(res[0], res[3], 5)
    got = mt.tally(nrules=5)
    same(got[0], want[0], "the next call answers: count")
    same(got[1], want[1], "the next call answers: lines")
    got = run_ids(hip, off, ids, 2)
    assert got[0].tolist() == [[1, 1, 1]] and got[1].tolist() == [[1, 1, 1]]


# ---- the real objects ------------------------------------------------------------------------------------------------------------

class Batch:
    """the first n of the 1 500 lines as a packed text on the device"""

    def __init__(self, rows, lens, n):
        self.data, self.off = lead_packed(rows[:n], lens[:n])
        self.n = n
        self.d_data, self.d_off = device_u8(self.data), device_u64(self.off)

    def device_args(self):
        return dict(d_base=self.d_data.data_ptr(), d_off=self.d_off.data_ptr(), n=self.n, limit=len(self.data))


def object_forms(hip, obj, off, ids, nrules, goff, what):
    """the device form and the host form of a matches or a tokens object against the judge over (off, ids)"""
    import torch
    want = tally_ref.tally(off, ids, nrules, goff)
    G = want[0].shape[0]
    d_goff = device_u64(goff) if goff is not None else None
    for which in ALL_FORMS:
        tabs = [Table(G, nrules + 1) if w else None for w in which]
        obj.tally_device(d_goff.data_ptr() if d_goff is not None else 0, G if goff is not None else 0, nrules,
                         tabs[0].ptr if tabs[0] else 0, tabs[1].ptr if tabs[1] else 0)
        torch.cuda.synchronize()
        for t, w, name in zip(tabs, want, ("count", "lines")):
            if t:
                same(t.read(), w, (what, "device", name, which))
    count, lines = obj.tally(goff, nrules)
    same(count, want[0], (what, "host", "count"))
    same(lines, want[1], (what, "host", "lines"))
    count, lines = obj.tally(goff, nrules, lines=False)
    assert lines is None
    same(count, want[0], (what, "host", "count alone"))
    return want


GROUPS = (None, [0, 8, 9, 9, 700, 1500], [3, 1400])


@pytest.mark.parametrize("flags", [0, DROP_EMPTY], ids=["all", "drop_empty"])
def test_matches_device_and_host_forms(hip, flags):
    for starts, ends, nrules in (("kw_starts", "kw_ends", 5), ("kw_starts", "kw_ends", 3), ("glob_first", "s15_start", 5), ("glob_first", "s15_start", 0)):
        rows, lens = inputs_of(ends)
        pd, td = starts_image(starts), ends_image(ends)
        res = reference(starts, ends, flags)
        for n in (257, 1500):
            r_off, _, _, r_id = matches_ref.head(res, n)
            b = Batch(rows, lens, n)
            mt = hip.HipMatches.run_device(pd, td, flags=flags, **b.device_args())
            assert mt.total == len(r_id)
            for goff in GROUPS:
                g = None if goff is None else np.minimum(np.array(goff, np.uint64), np.uint64(n))
                want = object_forms(hip, mt, r_off, r_id, nrules, g, (ends, nrules, n, flags, goff))
            mt.free()
        if ends == "kw_ends":                                               # line 8: 300 times d, rule 3, one line
            one = tally_ref.tally(res["off"], res["id"], 5, [8, 9])
            assert one[0].tolist() == [[0, 0, 0, 300, 0, 0]] and one[1].tolist() == [[0, 0, 0, 1, 0, 0]]
        else:                                                               # NO_ID alone: everything is "other"
            assert (res["id"] == NO_ID).all() and int(want[0][:, :nrules].sum()) == 0 and int(want[0].sum()) > 0
            assert ((res["end"] == res["start"]).sum() >= 100) == (flags == 0)


@functools.lru_cache(maxsize=None)
def tokens_reference():
    """(off, id) of the judge's tokens of the 1 500 keyword lines under SKIP_BAD, computed once"""
    rows, lens = inputs_of("kw_ends")
    res = tokens_ref.Judge(auto_of("kw_ends")[0], rows, lens).run(SKIP_BAD, state_ids("kw_ends"))
    res["off"].setflags(write=False)
    res["id"].setflags(write=False)
    return res["off"], res["id"]


def test_tokens_with_skip_bad(hip):
    """the tokens of the keyword lines: the bytes no keyword begins at are tokens of FSM_HIP_NO_MATCH, the other column"""
    rows, lens = inputs_of("kw_ends")
    td = ends_image("kw_ends")
    t_off, t_id = tokens_reference()
    assert (t_id == NO_MATCH).sum() > 1000 and set(t_id[t_id != NO_MATCH].tolist()) == set(range(5))
    for n in (257, 1500):
        b = Batch(rows, lens, n)
        tk = td.tokens_device(flags=SKIP_BAD, **b.device_args())
        off, ids = t_off[:n + 1], t_id[:int(t_off[n])]
        assert tk.total == len(ids)
        for goff in GROUPS:
            g = None if goff is None else np.minimum(np.array(goff, np.uint64), np.uint64(n))
            want = object_forms(hip, tk, off, ids, 5, g, ("tokens", n, goff))
        assert int(want[0][:, 5].sum()) > 0
        tk.close()


def test_matches_then_tokens_into_one_table(hip):
    """matches into a table, the tokens of the same lines on top with FSM_HIP_TALLY_ADD, device and host form"""
    import torch
    rows, lens = inputs_of("kw_ends")
    pd, td = starts_image("kw_starts"), ends_image("kw_ends")
    n = 1500
    b = Batch(rows, lens, n)
    res = reference("kw_starts", "kw_ends")
    t_off, t_id = tokens_reference()
    goff = np.array([0, 8, 9, 1000, 1500], np.uint64)
    m_want, t_want = tally_ref.tally(res["off"], res["id"], 5, goff), tally_ref.tally(t_off, t_id, 5, goff)
    mt = hip.HipMatches.run_device(pd, td, **b.device_args())
    tk = td.tokens_device(flags=SKIP_BAD, **b.device_args())
    d_goff = device_u64(goff)
    tabs = [Table(4, 6), Table(4, 6)]
    mt.tally_device(d_goff.data_ptr(), 4, 5, tabs[0].ptr, tabs[1].ptr)
    tk.tally_device(d_goff.data_ptr(), 4, 5, tabs[0].ptr, tabs[1].ptr, flags=hip.TALLY_ADD)
    torch.cuda.synchronize()
    for t, mw, tw, name in zip(tabs, m_want, t_want, ("count", "lines")):
        same(t.read(), mw + tw, ("device", name))
    both = tk.tally(goff, 5, add_to=mt.tally(goff, 5))
    same(both[0], m_want[0] + t_want[0], "host count")
    same(both[1], m_want[1] + t_want[1], "host lines")
    alone = tk.tally(goff, 5, add_to=(mt.tally(goff, 5)[0], None))
    assert alone[1] is None
    same(alone[0], m_want[0] + t_want[0], "host count alone")
    assert int(t_want[0][:, 5].sum()) > 0 and int(m_want[0][:, 5].sum()) == 0


def files_text(n, bounds, bare):
    """the first n keyword lines as files: file f is lines [bounds[f], bounds[f + 1]), every line followed by a newline except the
    last line of the files in `bare` -> (the text, file_off)"""
    rows, lens = inputs_of("kw_ends")
    files = []
    for f, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        parts = [bytes(rows[i, :lens[i]]) + b"\n" for i in range(a, b)]
        if f in bare:
            assert b > a and lens[b - 1] > 0                                # (an empty last line without a newline is no line)
            parts[-1] = parts[-1][:-1]
        files.append(b"".join(parts))
    return b"".join(files), np.concatenate([[0], np.cumsum([len(x) for x in files])]).astype(np.uint64)


def text_forms(hip, obj, text, hits, off, ids, goff, nfiles, what):
    """text_tally of a matches or a tokens object against the judge; -> the judge's tables at nrules = 5 and at nrules = 0"""
    import torch
    out = []
    for nrules in (5, 0):
        want = tally_ref.tally(off, ids, nrules, goff)
        assert want[0].shape == (nfiles, nrules + 1)
        for which in ALL_FORMS if nrules == 5 else ((True, True),):
            tabs = [Table(nfiles, nrules + 1) if w else None for w in which]
            obj.text_tally(text, hits, nrules, tabs[0].ptr if tabs[0] else 0, tabs[1].ptr if tabs[1] else 0)
            torch.cuda.synchronize()
            for t, w, name in zip(tabs, want, ("count", "lines")):
                if t:
                    same(t.read(), w, (what, nrules, name, which))
        out.append(want)
    return out


def test_a_text_of_files_with_and_without_hits(hip):
    """files through fsm_hip_text_open_files: empty files, files without a final delimiter, line 8 a file of its own.  The groups
    are the text's file_lines, or the hits' file_first; a plain text is one group"""
    from files_ref import files_ref
    n = 400
    rows, lens = inputs_of("kw_ends")
    bounds = [0, 0, 1, 8, 9, 9, 70, 200, 200, 399, 400, 400]
    bare = {f for f in (3, 5, 6, 9) if lens[bounds[f + 1] - 1] > 0}
    assert 3 in bare and len(bare) >= 3
    blob, fo = files_text(n, bounds, bare)
    nfiles = len(bounds) - 1
    t_off, file_lines = files_ref(blob, NL, fo)
    assert len(t_off) - 1 == n and file_lines.tolist() == bounds            # line i of the text is keyword line i
    pd, td = starts_image("kw_starts"), ends_image("kw_ends")
    res = reference("kw_starts", "kw_ends")
    r_off, _, _, r_id = matches_ref.head(res, n)
    per_line = np.diff(r_off.astype(np.int64))
    text = hip.HipText(blob, NL, file_off=fo)
    assert text.lines == n and text.files == nfiles
    mt = td.text_matches(pd, text)
    assert mt.count == n and mt.total == len(r_id)
    w5, w0 = text_forms(hip, mt, text, None, r_off, r_id, file_lines, nfiles, "files")
    totals = [int(per_line[a:b].sum()) for a, b in zip(bounds[:-1], bounds[1:])]
    assert w5[0].sum(axis=1).tolist() == totals and totals[3] == 300 and totals[0] == totals[4] == 0
    assert w0[1][:, 0].tolist() == [int((per_line[a:b] > 0).sum()) for a, b in zip(bounds[:-1], bounds[1:])]
    # the hits: the lines with a keyword, computed here; the matches of the hits are the selection of the judge's
    picks = np.flatnonzero(per_line > 0)
    ld = hip.LinesDfa(span_ref.line_matcher_of(KEYWORDS)[0], NL)
    hits = text.hits(ld)
    assert np.array_equal(hits.lines(), picks.astype(np.uint64)) and 100 < len(picks) < n
    s_off, _, _, s_id = matches_ref.select(res, picks)
    file_first = np.searchsorted(picks, bounds).astype(np.uint64)
    mh = td.text_matches(pd, text, hits)
    assert mh.count == len(picks)
    h5, h0 = text_forms(hip, mh, text, hits, s_off, s_id, file_first, nfiles, "hits")
    assert np.array_equal(h5[0], w5[0]) and np.array_equal(h5[1], w5[1])   # the lines without a match add nothing
    assert h0[1][:, 0].tolist() == np.diff(file_first.astype(np.int64)).tolist()
    # tokens of the same text, by file
    tk_off, tk_id = tokens_reference()
    tk = td.text_tokens(text, flags=SKIP_BAD)
    text_forms(hip, tk, text, None, tk_off[:n + 1], tk_id[:int(tk_off[n])], file_lines, nfiles, "tokens by file")
    # an object whose m is not the text's, or not the hits': EINVAL
    t = Table(nfiles, 6)
    for obj, h in ((mt, hits), (mh, None)):
        with pytest.raises(OSError) as ei:
            obj.text_tally(text, h, 5, t.ptr, 0)
        assert ei.value.errno == errno.EINVAL
    with pytest.raises(OSError) as ei:
        tk.text_tally(text, hits, 5, t.ptr, 0)
    assert ei.value.errno == errno.EINVAL
    assert (t.read() == FILL).all()
    # a plain text is one group
    whole = b"".join(bytes(rows[i, :lens[i]]) + b"\n" for i in range(n))
    plain = hip.HipText(whole, NL)
    assert plain.lines == n and plain.files == 0
    text_forms(hip, td.text_matches(pd, plain), plain, None, r_off, r_id, None, 1, "plain")


def test_example_prints_the_judges_counts(hip, tmp_path):
    """examples/hipcount.c over three small files, the last without a final newline: file:rule:matches:lines per file and rule with
    a match, -t for the totals, -r for fewer rules"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.RandomState(17)
    files = [[bytes(rng.choice(list(b"abcdxyzw" if i % 2 == 0 else b"xyzwba"), rng.randint(0, 25)).astype(np.uint8)) for i in range(k)] for k in (70, 40, 25)]
    files[2][-1] = b"xxabcabd"
    tables = []
    for nm, auto in (("starts", auto_of("kw_starts")[0]), ("ends", auto_of("kw_ends")[0])):
        tables.append(str(tmp_path / (nm + ".fsmhip")))
        auto[0].write_c(tables[-1])
    names = []
    for j, ls in enumerate(files):
        data = b"".join(x + b"\n" for x in ls)
        p = tmp_path / ("f%d.txt" % j)
        p.write_bytes(data[:-1] if j == 2 else data)
        names.append(str(p))
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    exe = str(tmp_path / "hipcount")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "hipcount.c"),
                           "-o", exe, "-L" + os.path.join(root, "libfsm_amd"), "-lfsm_hip", "-Wl,-rpath," + os.path.join(root, "libfsm_amd")])

    def run(*args, fs=names):
        r = subprocess.run([exe, *args, *tables, *fs], capture_output=True, env=env, timeout=120)
        return r.returncode, r.stdout

    def compose(nrules=5, totals=False, fs=(0, 1, 2)):
        lines = [x for j in fs for x in files[j]]
        rows, lens = span_ref.rows_of(lines)
        off, _, _, ids = judged("kw_starts", "kw_ends", rows, lens, DROP_EMPTY)
        goff = None if totals else np.concatenate([[0], np.cumsum([len(files[j]) for j in fs])])
        count, lin = tally_ref.tally(off, ids, nrules, goff)
        out = b""
        for g in range(count.shape[0]):
            for c in range(nrules + 1):
                if count[g, c]:
                    out += (b"" if totals else names[fs[g]].encode() + b":") + (b"%d" % c if c < nrules else b"other") + b":%d:%d\n" % (count[g, c], lin[g, c])
        return out

    want = compose()
    assert want.count(b"\n") >= 9 and b":other:" not in want
    assert run() == (0, want)
    assert run("-t") == (0, compose(totals=True))
    assert run("-r", "5") == (0, want)
    fewer = compose(3)
    assert fewer.count(b":other:") == 3
    assert run("-r", "3") == (0, fewer)
    assert run("-t", "-r", "0") == (0, compose(0, True)) and compose(0, True).startswith(b"other:")
    assert run(fs=[names[2], names[0]]) == (0, compose(fs=(2, 0)))
    quiet = tmp_path / "none.txt"
    quiet.write_bytes(b"xyz\nwwww\n\n")
    assert run(fs=[str(quiet)]) == (1, b"")
    assert run(fs=[names[1], str(quiet)]) == (0, compose(fs=(1,)))
