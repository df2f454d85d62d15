"""CPU: the files entry points of the text front (include/fsm_hip.h, "Files of a text") fail LOUDLY without a device, their
accessors take NULL, and the two statements of the rule (tests/files_ref.py) agree.  tests/test_abi.py's export check covers
the declarations themselves."""
import ctypes as C
import errno

import numpy as np
import pytest


def lib_of():
    from libfsm_amd import load_library
    lib = load_library()
    return lib


@pytest.mark.parametrize("delim", [0x0A, 0x00], ids=["0x0a", "0x00"])
def test_the_two_statements_of_the_rule_agree(delim):
    """the union form against "each file cut alone, shifted and concatenated": random buffers, empty files at the start, in the
    middle and at the end"""
    from files_ref import files_ref, files_ref_each
    from text_ref import split_ref
    rng = np.random.RandomState(delim + 1)
    for case in range(200):
        nbytes = int(rng.randint(0, 120))
        density = (2, 5, 40)[case % 3]
        buf = np.where(rng.randint(0, density, nbytes) == 0, delim, rng.randint(1, 256, nbytes)).astype(np.uint8)
        inner = np.sort(rng.randint(0, nbytes + 1, rng.randint(0, 12)))
        fo = np.concatenate([[0] * (1 + case % 3), inner, np.repeat(inner[:2], 2), [nbytes] * (1 + case // 3 % 3)])
        fo = np.sort(fo).astype(np.uint64)
        off, fl = files_ref(buf, delim, fo)
        off2, fl2 = files_ref_each(buf, delim, fo)
        assert np.array_equal(off, off2) and np.array_equal(fl, fl2), (case, bytes(buf), fo)
        assert off[0] == 0 and off[-1] == nbytes and (np.diff(off.astype(np.int64)) > 0).all()
        assert fl[0] == 0 and fl[-1] == len(off) - 1 and np.array_equal(off[fl.astype(np.int64)], fo)
        assert set(split_ref(buf, delim).tolist()) <= set(off.tolist())


def test_a_case_to_check_by_eye():
    from files_ref import files_ref, files_ref_each, hits_ref_off, join_files
    buf, fo = join_files([b"ab\ncd", b"", b"ef\n\ngh\n", b"\nij"])
    assert bytes(buf) == b"ab\ncdef\n\ngh\n\nij" and fo.tolist() == [0, 5, 5, 12, 15]
    off, fl = files_ref(buf, 0x0A, fo)
    # lines: "ab\n", "cd" | (none) | "ef\n", "\n", "gh\n" | "\n", "ij"
    assert off.tolist() == [0, 3, 5, 8, 9, 12, 13, 15] and fl.tolist() == [0, 2, 2, 5, 7]
    off2, fl2 = files_ref_each(buf, 0x0A, fo)
    assert off2.tolist() == off.tolist() and fl2.tolist() == fl.tolist()
    lines, out_off, out = hits_ref_off(buf, off, [False, True, False, False, True, False, True])
    assert lines.tolist() == [1, 4, 6] and out_off.tolist() == [0, 2, 5, 7] and bytes(out) == b"cdgh\nij"
    assert np.searchsorted(lines, fl).tolist() == [0, 1, 1, 2, 3]     # file_first: one hit in file 0, none in 1, one in 2, one in 3


def test_no_files_text_without_a_device(built):
    """no CPU path: NULL + ENODEV from both forms, also with arguments that a device would call EINVAL"""
    import torch
    import libfsm_amd
    lib = lib_of()
    text = np.frombuffer(b"ab\ncd", np.uint8)
    good, bad = np.array([0, 3, 5], np.uint64), np.array([1, 3, 5], np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert libfsm_amd.text_files_block() >= 64
    if torch.cuda.is_available():
        for fo, nfiles in ((bad, 2), (good, 0), (None, 2)):
            C.set_errno(0)
            assert lib.fsm_hip_text_open_files(vp(text), C.c_size_t(5), 0x0A, vp(fo) if fo is not None else None, C.c_size_t(nfiles)) is None
            assert C.get_errno() == errno.EINVAL
        return
    for fo, nfiles in ((good, 2), (bad, 2), (good, 0), (None, 2)):
        p = vp(fo) if fo is not None else None
        C.set_errno(0)
        assert lib.fsm_hip_text_open_files(vp(text), C.c_size_t(5), 0x0A, p, C.c_size_t(nfiles)) is None
        assert C.get_errno() == errno.ENODEV
        C.set_errno(0)
        assert lib.fsm_hip_text_open_files_device(vp(text), C.c_size_t(5), 0x0A, p, C.c_size_t(nfiles), None) is None
        assert C.get_errno() == errno.ENODEV
    with pytest.raises(OSError) as ei:
        libfsm_amd.HipText(b"ab\ncd", 0x0A, file_off=good)
    assert ei.value.errno == errno.ENODEV
    with pytest.raises(OSError) as ei:
        libfsm_amd.HipText(d_text=text.ctypes.data, nbytes=5, delim=0x0A, file_off=good.ctypes.data, nfiles=2)
    assert ei.value.errno == errno.ENODEV


def test_accessors_take_null(built):
    lib = lib_of()
    out = np.zeros(4, np.uint64)
    assert lib.fsm_hip_text_files(None) == 0
    assert lib.fsm_hip_text_file_lines_device(None) is None and lib.fsm_hip_text_hits_file_first_device(None) is None
    for fn in (lib.fsm_hip_text_file_lines, lib.fsm_hip_text_hits_file_first):
        C.set_errno(0)
        assert fn(None, out.ctypes.data_as(C.c_void_p)) == -1 and C.get_errno() == errno.EINVAL
    for fn in (lib.fsm_hip_text_files_ms, lib.fsm_hip_text_hits_file_first_ms):
        C.set_errno(0)
        assert fn(None) == -1.0 and C.get_errno() == errno.EINVAL
    assert lib.fsm_hip_text_files_block() % 64 == 0
