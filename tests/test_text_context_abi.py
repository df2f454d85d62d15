"""CPU: the context entry points of the text front (include/fsm_hip.h, "Context") fail LOUDLY without a device, their accessors
take NULL, the two statements of the rule (tests/context_ref.py) agree, and the composer reproduces three GNU grep 3.7
transcripts.  tests/test_abi.py's export check covers the declarations themselves."""
import ctypes as C
import errno

import numpy as np
import pytest

ALL = 2 ** 64 - 1


def lib_of():
    from libfsm_amd import load_library
    lib = load_library()
    return lib


def random_case(rng, case):
    """n in 0..200, one line in 2 / 10 / 100 selected, every other case a text of files with empty files at the start, in the
    middle and at the end"""
    n = int(rng.randint(0, 201))
    sel = rng.randint(0, (2, 10, 100)[case % 3], n) == 0
    fl = None
    if case % 2:
        inner = np.sort(rng.randint(0, n + 1, rng.randint(0, 9)))
        fl = np.sort(np.concatenate([[0] * (1 + case % 3), inner, np.repeat(inner[:2], 2), [n] * (1 + case // 3 % 3)])).astype(np.uint64)
    return n, sel, fl


def test_the_two_statements_of_the_rule_agree():
    from context_ref import context_literal, context_witness, file_of, marks_ref
    rng = np.random.RandomState(5)
    seen_files = seen_cut = 0
    for case in range(400):
        n, sel, fl = random_case(rng, case)
        choices = [0, 1, 2, 5, n, ALL]
        before = choices[rng.randint(len(choices))]
        after = choices[rng.randint(len(choices))]
        while after == before:
            after = choices[rng.randint(len(choices))]
        W = context_literal(sel, before, after, fl)
        assert np.array_equal(W, context_witness(sel, before, after, fl)), (case, n, before, after, fl)
        assert (W | ~sel).all() and (W.any() == sel.any())                   # S is inside W; no selected line, no hit
        fo = file_of(n, fl)
        for j in np.unique(fo[W]):                                           # a file has hits only if it has a selected line
            assert sel[fo == j].any()
        lines, core, group = marks_ref(sel, W, fl)
        assert int(core.sum()) == int(sel.sum()) and (len(lines) == 0 or group[0])
        if fl is not None:
            seen_files += 1
            seen_cut += int(not np.array_equal(W, context_literal(sel, before, after)))
    assert seen_files >= 150 and seen_cut >= 30                              # the file ends did cut contexts


def test_zero_context_is_the_plain_selection():
    from context_ref import context_literal, marks_ref
    sel = np.array([1, 1, 0, 1, 0, 0, 1, 1, 1], bool)
    W = context_literal(sel, 0, 0)
    assert np.array_equal(W, sel)
    lines, core, group = marks_ref(sel, W)
    assert core.all() and group.tolist() == [True, False, True, True, False, False]
    lines, core, group = marks_ref(sel, W, [0, 1, 1, 8, 9])                  # a file start between two neighbours begins a group
    assert group.tolist() == [True, True, True, True, False, True]


A, B, CC = [b"x", b"m", b"x"], [b"x", b"m"], [b"m", b"x", b"x", b"x", b"m", b"m", b"x"]

GREP_H_N_A1_B1 = b"""a-1-x
a:2:m
a-3-x
--
b-1-x
b:2:m
--
c:1:m
c-2-x
--
c-4-x
c:5:m
c:6:m
c-7-x
"""


def test_three_gnu_grep_transcripts():
    """GNU grep 3.7 over a = "x\\nm\\nx\\n", b = "x\\nm\\n", c = "m\\nx\\nx\\nx\\nm\\nm\\nx" (no final newline)"""
    from context_ref import compose
    is_m = lambda ls: [l == b"m" for l in ls]   # noqa: E731
    # grep -H -n -A1 -B1 m a b c
    assert compose([b"a", b"b", b"c"], [A, B, CC], [is_m(A), is_m(B), is_m(CC)], 1, 1) == GREP_H_N_A1_B1
    # grep -n -v -A1 m c
    assert compose([b"c"], [CC], [[not s for s in is_m(CC)]], 0, 1, with_name=False) == b"2:x\n3:x\n4:x\n5-m\n--\n7:x\n"
    # grep -n -B2 m c
    assert compose([b"c"], [CC], [is_m(CC)], 2, 0, with_name=False) == b"1:m\n--\n3-x\n4-x\n5:m\n6:m\n"


def test_no_context_hits_without_a_device(built):
    """no CPU path: NULL + ENODEV from both forms whatever the arguments; with a device a NULL text or flags 4 give EINVAL"""
    import torch
    lib = lib_of()
    bitmap = np.zeros(1, np.uint64)
    u64 = C.c_uint64
    want = errno.EINVAL if torch.cuda.is_available() else errno.ENODEV
    for flags in (0, 1, 2, 3, 4):
        for before, after in ((0, 0), (1, 2), (ALL, ALL)):
            C.set_errno(0)
            assert lib.fsm_hip_text_hits_context(None, None, C.c_uint(flags), u64(before), u64(after)) is None
            assert C.get_errno() == want
            C.set_errno(0)
            assert lib.fsm_hip_text_hits_context_device(None, bitmap.ctypes.data_as(C.c_void_p), C.c_uint(flags), u64(before), u64(after), None) is None
            assert C.get_errno() == want
    if torch.cuda.is_available():
        import libfsm_amd
        ht = libfsm_amd.HipText(b"a\nb\n", 0x0A)
        d_bm = torch.zeros(1, dtype=torch.int64, device="cuda")
        for flags in (4, 8, 5):
            with pytest.raises(OSError) as ei:
                ht.hits_context_device(d_bm.data_ptr(), 1, 1, flags=flags)
            assert ei.value.errno == errno.EINVAL
        with pytest.raises(OSError) as ei:
            ht.hits_context_device(0, 1, 1)
        assert ei.value.errno == errno.EINVAL
        ht.close()


def test_accessors_take_null(built):
    import libfsm_amd
    lib = lib_of()
    out = np.zeros(4, np.uint64)
    assert lib.fsm_hip_text_hits_core_device(None) is None and lib.fsm_hip_text_hits_group_device(None) is None
    assert lib.fsm_hip_text_hits_core_count(None) == 0 and lib.fsm_hip_text_hits_groups(None) == 0
    C.set_errno(0)
    assert lib.fsm_hip_text_hits_marks(None, out.ctypes.data_as(C.c_void_p), None) == -1 and C.get_errno() == errno.EINVAL
    C.set_errno(0)
    assert lib.fsm_hip_text_hits_context_ms(None) == -1.0 and C.get_errno() == errno.EINVAL
    assert lib.fsm_hip_text_context_scan_block() >= 64 and lib.fsm_hip_text_context_scan_block() % 64 == 0
    assert libfsm_amd.text_context_scan_block() == lib.fsm_hip_text_context_scan_block()
