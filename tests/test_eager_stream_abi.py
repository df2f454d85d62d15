"""CPU: the eager-output streaming fronts are exported by libfsm_hip.so and refuse bad arguments before touching a device."""
import ctypes as C
import errno as _errno

import pytest

NEW = ("fsm_hip_exec_batch_eager_resume", "fsm_hip_exec_batch_eager_resume_device",
       "fsm_hip_match_buffer_big_eager", "fsm_hip_match_file_eager")


@pytest.fixture(scope="module")
def lib(built):
    import libfsm_amd
    return libfsm_amd.load_library()


def test_new_symbols_exported(lib):
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing


def test_null_dfa_is_einval(lib):
    vp = C.c_void_p
    st = (C.c_uint32 * 1)(0xFFFFFFFD)
    eo = (C.c_uint64 * 1)(0)
    buf = C.create_string_buffer(b"abc")
    calls = [
        lambda: lib.fsm_hip_exec_batch_eager_resume(None, buf, C.c_size_t(3), None, None, C.c_size_t(1), st, None, eo),
        lambda: lib.fsm_hip_exec_batch_eager_resume_device(None, buf, C.c_size_t(3), None, None, C.c_size_t(1), st, None, eo, None),
        lambda: lib.fsm_hip_match_buffer_big_eager(None, buf, C.c_size_t(3), None, eo),
        lambda: lib.fsm_hip_match_file_eager(None, vp(None), None, eo),
    ]
    for k, call in enumerate(calls):
        C.set_errno(0)
        assert call() == -1, NEW[k]
        assert C.get_errno() == _errno.EINVAL, NEW[k]
