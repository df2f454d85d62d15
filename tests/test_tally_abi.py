"""CPU: the tally (include/fsm_hip.h, "tally").  The judge of tests/tally_ref.py against three-line Python loops on small random
cases, and the entry points: declared, exported, in the binding's table, failing LOUDLY without a device."""
import ctypes as C
import errno
import os

import numpy as np
import pytest

import tally_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("fsm_hip_tally_ids_device", "fsm_hip_matches_tally_device", "fsm_hip_tokens_tally_device", "fsm_hip_matches_tally",
           "fsm_hip_tokens_tally", "fsm_hip_text_matches_tally", "fsm_hip_text_tokens_tally", "fsm_hip_tally_span_inputs",
           "fsm_hip_tally_window", "fsm_hip_tally_lds_columns", "fsm_hip_tally_max_line_columns")


def loops(off, ids, nrules, group_off):
    """the definition, entry by entry"""
    m, total, C = len(off) - 1, len(ids), nrules + 1
    G = 1 if group_off is None else len(group_off) - 1
    count, lines = np.zeros((G, C), np.uint64), np.zeros((G, C), np.uint64)
    for j in range(m):
        gs = [0] if group_off is None else [g for g in range(G) if group_off[g] <= j < group_off[G]]
        cols = [int(ids[k]) if ids[k] < nrules else nrules for k in range(min(int(off[j]), total), min(int(off[j + 1]), total))]
        for c in cols if gs else []:
            count[gs[-1], c] += 1
        for c in set(cols) if gs else []:
            lines[gs[-1], c] += 1
    return count, lines


def test_judge_is_the_loops():
    rng = np.random.RandomState(7)
    seen_other = seen_empty_group = seen_nowhere = 0
    for case in range(200):
        m = rng.randint(0, 30)
        nrules = (0, 1, 5, 40)[case % 4]
        off = np.concatenate([[rng.randint(0, 3)], np.cumsum(rng.choice([0, 0, 1, 2, 9, 40], m))]).astype(np.uint64)
        off[1:] += off[0]
        total = int(off[-1]) - (rng.randint(0, 5) if case % 5 == 0 else 0)
        ids = rng.randint(0, nrules + 3, max(total, 0)).astype(np.uint32)
        ids[rng.rand(len(ids)) < 0.1] = tally_ref.NO_MATCH
        ids[rng.rand(len(ids)) < 0.1] = tally_ref.NO_ID
        goff = None
        if case % 3:
            goff = np.sort(rng.randint(0, m + 1, rng.randint(2, 9))).astype(np.uint64)
            seen_empty_group += int((np.diff(goff.astype(np.int64)) == 0).any())
            seen_nowhere += int(goff[0] > 0 or goff[-1] < m)
        seen_other += int((ids >= nrules).any())
        count, lines = tally_ref.tally(off, ids, nrules, goff)
        w_count, w_lines = loops(off, ids, nrules, goff)
        assert np.array_equal(count, w_count) and np.array_equal(lines, w_lines), case
        assert count.dtype == lines.dtype == np.uint64 and count.shape == lines.shape == (1 if goff is None else len(goff) - 1, nrules + 1)
        assert (lines <= count).all()
    assert seen_other > 50 and seen_empty_group > 20 and seen_nowhere > 20


def test_judge_on_a_case_by_hand():
    # inputs: 0 = [3, 3, 9], 1 = [], 2 = [0, NO_ID], 3 = [1]; two rules, so 3, 9 and NO_ID are "other"
    off, ids = [0, 3, 3, 5, 6], [3, 3, 9, 0, tally_ref.NO_ID, 1]
    count, lines = tally_ref.tally(off, ids, 2)
    assert count.tolist() == [[1, 1, 4]] and lines.tolist() == [[1, 1, 2]]
    # groups: [0, 0) empty, [0, 3), [3, 3) empty; input 3 is counted nowhere
    count, lines = tally_ref.tally(off, ids, 2, [0, 0, 3, 3])
    assert count.tolist() == [[0, 0, 0], [1, 0, 4], [0, 0, 0]] and lines.tolist() == [[0, 0, 0], [1, 0, 2], [0, 0, 0]]
    # no rule: one column, the number of entries and of inputs with an entry
    count, lines = tally_ref.tally(off, ids, 0)
    assert count.tolist() == [[6]] and lines.tolist() == [[3]]
    assert tally_ref.col([0, 4, 5, tally_ref.NO_MATCH], 5).tolist() == [0, 4, 5, 5]


def test_every_new_symbol_is_declared_exported_and_in_the_table(built):
    import libfsm_amd
    from libfsm_amd import capi
    from test_abi import declared_symbols
    lib = libfsm_amd.load_library()
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert [s for s in SYMBOLS if s not in capi.PROTOTYPES] == []
    assert [s for s in SYMBOLS if s not in declared_symbols()] == []
    assert libfsm_amd.TALLY_ADD == tally_ref.ADD == 1
    for cls in (libfsm_amd.HipMatches, libfsm_amd.HipTokens):
        for name in ("tally", "tally_device", "text_tally"):
            assert callable(getattr(cls, name))
    assert callable(libfsm_amd.tally_ids_device)
    # the constants need no device: a window is a workgroup of 256, the LDS counters and the bitmap are powers of two
    assert libfsm_amd.tally_window() == 256 and libfsm_amd.tally_span_inputs() >= 1
    assert 1024 < libfsm_amd.tally_lds_columns() < libfsm_amd.tally_max_line_columns() <= 1 << 20
    assert libfsm_amd.tally_max_line_columns() % 32 == 0


def test_no_tally_without_a_device(built):
    """no CPU path: ENODEV from every entry point, whatever the arguments (with a device, these arguments are EINVAL)"""
    import torch
    import libfsm_amd
    want = errno.EINVAL if torch.cuda.is_available() else errno.ENODEV
    lib = libfsm_amd.load_library()
    out = np.zeros(4, np.uint64)
    p = out.ctypes.data_as(C.c_void_p)
    for fn, args in ((lib.fsm_hip_tally_ids_device, (None, None, 1, 1, None, 0, 1, 0, None, None, None)),
                     (lib.fsm_hip_tally_ids_device, (None, None, 0, 0, None, 0, 1, 2, p, None, None)),
                     (lib.fsm_hip_matches_tally_device, (None, None, 0, 1, 0, p, None, None)),
                     (lib.fsm_hip_tokens_tally_device, (None, None, 0, 1, 0, p, None, None)),
                     (lib.fsm_hip_matches_tally, (None, None, 0, 1, 0, p, None)),
                     (lib.fsm_hip_tokens_tally, (None, None, 0, 1, 0, None, p)),
                     (lib.fsm_hip_text_matches_tally, (None, None, None, 1, 0, p, None, None)),
                     (lib.fsm_hip_text_tokens_tally, (None, None, None, 1, 0, p, None, None))):
        C.set_errno(0)
        assert fn(*args) == -1 and C.get_errno() == want
    assert (out == 0).all()
    if not torch.cuda.is_available():
        with pytest.raises(OSError) as ei:
            libfsm_amd.tally_ids_device(0, 0, 0, 0, 0, 0, 1, out.ctypes.data, 0)
        assert ei.value.errno == errno.ENODEV
