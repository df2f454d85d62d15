"""CPU: the hits entry points of the text front (include/fsm_hip.h, "The hits") fail LOUDLY without a device and their
accessors take NULL.  tests/test_abi.py's export check covers the declarations themselves."""
import ctypes as C
import errno

import numpy as np


def lib_of():
    from libfsm_amd import load_library
    lib = load_library()
    return lib


def test_no_hits_without_a_device(built):
    """no CPU path: NULL + ENODEV from both forms, whatever the arguments (with a device, the NULL text is EINVAL)"""
    import torch
    want = errno.EINVAL if torch.cuda.is_available() else errno.ENODEV
    lib = lib_of()
    bitmap = np.zeros(1, np.uint64)
    for flags in (0, 1, 2, 3):
        C.set_errno(0)
        assert lib.fsm_hip_text_hits(None, None, C.c_uint(flags)) is None
        assert C.get_errno() == want
        C.set_errno(0)
        assert lib.fsm_hip_text_hits_device(None, bitmap.ctypes.data_as(C.c_void_p), C.c_uint(flags), None) is None
        assert C.get_errno() == want


def test_python_front_raises_without_a_device(built):
    import pytest
    import torch
    import libfsm_amd
    assert libfsm_amd.HITS_INVERT == 1 and libfsm_amd.HITS_NO_BYTES == 2
    assert libfsm_amd.text_hits_block_lines() >= 64 and libfsm_amd.text_hits_block_lines() % 64 == 0
    assert libfsm_amd.text_hits_block_bytes() >= 16 and libfsm_amd.text_hits_block_bytes() % 16 == 0
    if not torch.cuda.is_available():
        with pytest.raises(OSError) as ei:
            libfsm_amd.HipText(b"a\nb\n", 0x0A)
        assert ei.value.errno == errno.ENODEV


def test_accessors_take_null(built):
    lib = lib_of()
    assert lib.fsm_hip_text_hits_count(None) == 0 and lib.fsm_hip_text_hits_nbytes(None) == 0
    for f in ("lines_device", "offsets_device", "bytes_device"):
        fn = getattr(lib, "fsm_hip_text_hits_" + f)
        assert fn(None) is None
    out = np.zeros(4, np.uint64)
    C.set_errno(0)
    assert lib.fsm_hip_text_hits_copy(None, out.ctypes.data_as(C.c_void_p), None, None) == -1 and C.get_errno() == errno.EINVAL
    C.set_errno(0)
    assert lib.fsm_hip_text_hits_ms(None) == -1.0 and C.get_errno() == errno.EINVAL
    assert lib.fsm_hip_text_hits_gather_ms(None) == -1.0
    lib.fsm_hip_text_hits_free(None)     # as free(NULL)


def test_reference_rule():
    """tests/hits_ref.py on a text small enough to check by eye"""
    from hits_ref import hits_ref, pack_bits
    text = b"ab\n\ncde\nf"           # lines: "ab\n", "\n", "cde\n", "f" (no delimiter)
    lines, off, out = hits_ref(text, 0x0A, [True, False, True, True])
    assert lines.tolist() == [0, 2, 3] and off.tolist() == [0, 3, 7, 8] and bytes(out) == b"ab\ncde\nf"
    lines, off, out = hits_ref(text, 0x0A, [True, False, True, True], invert=True)
    assert lines.tolist() == [1] and off.tolist() == [0, 1] and bytes(out) == b"\n"
    lines, off, out = hits_ref(b"", 0x0A, [])
    assert lines.tolist() == [] and off.tolist() == [0] and len(out) == 0
    assert pack_bits([True, False, True]).tolist() == [5] and pack_bits([True, False, True], 1).tolist() == [2 ** 64 - 1 - 2]
    assert len(pack_bits(np.ones(65, bool))) == 2 and len(pack_bits([])) == 0
