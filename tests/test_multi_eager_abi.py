"""CPU: the many-DFA front's eager-output entry points are exported, declared in include/fsm_hip.h, bound in libfsm_amd, keep the
layout of the job structs beside them, and refuse bad arguments before touching a device."""
import ctypes as C
import errno as _errno
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fsm_hip_exec_multi_eager", "fsm_hip_exec_multi_eager_device", "fsm_hip_multi_prepare_eager")


@pytest.fixture(scope="module")
def lib(built):
    import libfsm_amd
    return libfsm_amd.load_library()


def test_new_symbols_exported_and_declared(lib):
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing
    header = open(os.path.join(ROOT, "include", "fsm_hip.h")).read()
    for s in NEW:
        assert re.search(r"^int %s\(const struct fsm_hip_dfa \*const \*dfa, const struct fsm_hip_multi_batch_eager \*b, size_t k, int ids_mode" % s, header, re.M), s
    body = re.search(r"struct fsm_hip_multi_batch_eager \{(.*?)\};", header, re.S).group(1)
    fields = re.findall(r"\*?(\w+);", body)
    assert fields == ["base", "off", "n", "end_out", "accept_bitmap", "id_out", "eager_out"]


def test_python_names_and_struct_layout(built):
    import libfsm_amd as hip
    for name in ("MultiBatchEager", "exec_multi_eager", "exec_multi_eager_device", "MultiPrepared"):
        assert hasattr(hip, name), name
    word = C.sizeof(C.c_void_p)
    assert C.sizeof(C.c_size_t) == word
    assert C.sizeof(hip.MultiBatchEager) == 7 * word
    assert [f[0] for f in hip.MultiBatchEager._fields_] == ["base", "off", "n", "end_out", "accept_bitmap", "id_out", "eager_out"]
    assert hip.MultiBatchEager.eager_out.offset == 6 * word
    # the two structs beside it are what they were
    assert C.sizeof(hip.MultiBatchIds) == 6 * word
    assert C.sizeof(hip.MultiBatch) == 5 * word


def test_null_arguments_are_einval(lib):
    import libfsm_amd as hip
    one_null_dfa = (C.c_void_p * 1)(None)
    jobs = (hip.MultiBatchEager * 1)()
    out = C.c_void_p()
    k = C.c_size_t(1)
    calls = {
        "exec_multi_eager(NULL dfa)": lambda: lib.fsm_hip_exec_multi_eager(None, jobs, k, C.c_int(1)),
        "exec_multi_eager(NULL b)": lambda: lib.fsm_hip_exec_multi_eager(one_null_dfa, None, k, C.c_int(1)),
        "exec_multi_eager_device(NULL dfa)": lambda: lib.fsm_hip_exec_multi_eager_device(None, jobs, k, C.c_int(1), None),
        "exec_multi_eager_device(NULL b)": lambda: lib.fsm_hip_exec_multi_eager_device(one_null_dfa, None, k, C.c_int(1), None),
        "multi_prepare_eager(NULL dfa)": lambda: lib.fsm_hip_multi_prepare_eager(None, jobs, k, C.c_int(1), C.byref(out)),
        "multi_prepare_eager(NULL b)": lambda: lib.fsm_hip_multi_prepare_eager(one_null_dfa, None, k, C.c_int(1), C.byref(out)),
        "multi_prepare_eager(NULL out)": lambda: lib.fsm_hip_multi_prepare_eager(one_null_dfa, jobs, k, C.c_int(1), None),
        "multi_prepare_eager(NULL out, k = 0)": lambda: lib.fsm_hip_multi_prepare_eager(None, None, C.c_size_t(0), C.c_int(1), None),
    }
    for what, call in calls.items():
        C.set_errno(0)
        assert call() == -1, what
        assert C.get_errno() == _errno.EINVAL, what
    assert not out.value


def test_empty_submission_is_zero(lib):
    assert lib.fsm_hip_exec_multi_eager(None, None, C.c_size_t(0), C.c_int(1)) == 0
    assert lib.fsm_hip_exec_multi_eager_device(None, None, C.c_size_t(0), C.c_int(1), None) == 0
    out = C.c_void_p()
    assert lib.fsm_hip_multi_prepare_eager(None, None, C.c_size_t(0), C.c_int(1), C.byref(out)) == 0
    assert out.value
    lib.fsm_hip_multi_prepared_free(out)
    import libfsm_amd as hip
    assert hip.exec_multi_eager([], []) == []
