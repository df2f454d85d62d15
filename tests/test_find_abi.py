"""CPU: the lookup of a packed text's records among the keys of a distinct object (include/fsm_hip.h, "find").  The judge of
tests/find_ref.py on cases by hand, and the entry points: declared, exported, in the binding's table, failing LOUDLY without a
device -- ENODEV before any argument check; with a device the same arguments are refused for what they are."""
import ctypes as C
import errno

import numpy as np
import pytest

import find_ref
from distinct_ref import pack

SYMBOLS = ("fsm_hip_keys_find_device", "fsm_hip_keys_find", "fsm_hip_keys_find_extracted", "fsm_hip_keys_find_hits", "fsm_hip_keys_find_text",
           "fsm_hip_found_records", "fsm_hip_found_present", "fsm_hip_found_class_device", "fsm_hip_found_bitmap_device", "fsm_hip_found_pick_device",
           "fsm_hip_found_copy", "fsm_hip_found_ms", "fsm_hip_found_pass_ms", "fsm_hip_found_free")
NL = 0x0A
NONE = find_ref.NONE


def test_judge_on_cases_by_hand():
    keys = find_ref.numbers_of(*pack([b"a\n", b"b", b"a", b"cc\n"]), trim=NL)
    assert keys == {(b"a", 0): 0, (b"b", 0): 1, (b"cc", 0): 2}
    # the probe trims for itself: with its own trim "a\n" is the key a, without it is not
    cls, bitmap, pick, present = find_ref.find(keys, *pack([b"a\n", b"x", b"cc", b"b\n\n", b"b\n"]), trim=NL)
    assert cls.tolist() == [0, NONE, 2, NONE, 1] and bitmap.tolist() == [0b10101] and pick.tolist() == [0, 2, 4, 1, 3] and present == 3
    cls, bitmap, pick, present = find_ref.find(keys, *pack([b"a\n", b"a"]), trim=-1)
    assert cls.tolist() == [NONE, 0] and bitmap.tolist() == [2] and pick.tolist() == [1, 0] and present == 1
    # trim on the dictionary's side only: its keys keep nothing of the byte, the probe's records keep theirs
    keys = find_ref.numbers_of(*pack([b"a;", b"b"]), trim=ord(";"))
    assert find_ref.find(keys, *pack([b"a;", b"a", b"b;"]), trim=-1)[0].tolist() == [NONE, 0, NONE]
    assert find_ref.find(keys, *pack([b"a;", b"a", b"b;"]), trim=ord(";"))[0].tolist() == [0, 0, 1]
    # tags: equal bytes under another tag are absent; no tag array is tag 0, on either side
    keys = find_ref.numbers_of(*pack([b"x", b"x", b"y"]), tag=[1, 0, 2])
    assert find_ref.find(keys, *pack([b"x", b"x", b"x", b"y", b"y"]), tag=[0, 1, 2, 2, 0])[0].tolist() == [1, 0, NONE, 2, NONE]
    assert find_ref.find(keys, *pack([b"x", b"y"]))[0].tolist() == [1, NONE]
    keys = find_ref.numbers_of(*pack([b"x", b"y"]))
    assert find_ref.find(keys, *pack([b"x", b"y"]), tag=[0, 7])[0].tolist() == [0, NONE]
    # offsets are clamped to the bytes that may be read and to their predecessor, on both sides
    keys = find_ref.numbers_of([0, 2, 1, 9], b"abcd", nbytes=3)
    assert keys == {(b"ab", 0): 0, (b"", 0): 1, (b"bc", 0): 2}
    cls, _, pick, present = find_ref.find(keys, [0, 2, 4, 3, 8], b"bcabab", nbytes=5)
    assert cls.tolist() == [2, 0, 1, NONE] and pick.tolist() == [0, 1, 2, 3] and present == 3
    # the empty key, present and absent
    assert find_ref.find(find_ref.numbers_of(*pack([b"a", b"\n"]), trim=NL), *pack([b"", b"\n", b"\n\n"]), trim=NL)[0].tolist() == [1, 1, NONE]
    assert find_ref.find(find_ref.numbers_of(*pack([b"a"]), trim=NL), *pack([b"", b"\n"]), trim=NL)[0].tolist() == [NONE, NONE]
    # no probe record; no key
    cls, bitmap, pick, present = find_ref.find(keys, [0], b"")
    assert len(cls) == len(bitmap) == len(pick) == 0 and present == 0
    cls, bitmap, pick, present = find_ref.find(find_ref.numbers_of([0], b""), *pack([b"a"] * 65))
    assert (cls == NONE).all() and bitmap.tolist() == [0, 0] and pick.tolist() == list(range(65)) and present == 0
    # the tail of the last bitmap word is 0
    cls, bitmap, pick, present = find_ref.find(find_ref.numbers_of(*pack([b"a"])), *pack([b"a"] * 65))
    assert bitmap.tolist() == [2 ** 64 - 1, 1] and present == 65 and pick.tolist() == list(range(65))


def test_every_new_symbol_is_declared_exported_and_in_the_table(built):
    import libfsm_amd
    from libfsm_amd import capi
    from test_abi import declared_symbols
    lib = libfsm_amd.load_library()
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert [s for s in SYMBOLS if s not in capi.PROTOTYPES] == []
    assert sorted(s for s in declared_symbols() if "find" in s or "found" in s) == sorted(SYMBOLS)
    assert [s for s in SYMBOLS if "distinct" in s or "sort" in s] == []
    assert libfsm_amd.FIND_NO_PICK == find_ref.NO_PICK == 1 and libfsm_amd.FOUND_NONE == find_ref.NONE == 0xFFFFFFFF
    for name in ("records", "present", "class_ptr", "bitmap_ptr", "pick_ptr", "copy", "ms", "pass_ms", "free"):
        assert hasattr(libfsm_amd.HipFound, name), name
    for name in ("find_device", "find", "find_extracted", "find_hits", "find_text"):
        assert callable(getattr(libfsm_amd.HipDistinct, name)), name


def test_no_find_without_a_device(built):
    """no CPU path: ENODEV from every entry point before any argument check (with a device, these arguments are EINVAL)"""
    import torch
    import libfsm_amd
    have = torch.cuda.is_available()
    lib = libfsm_amd.load_library()
    off = np.zeros(2, np.uint64)
    down = np.array([0, 3, 2], np.uint64)
    p, d = off.ctypes.data_as(C.c_void_p), down.ctypes.data_as(C.c_void_p)
    abc = C.c_char_p(b"abc")
    for fn, args in ((lib.fsm_hip_keys_find_device, (None, None, None, 1, 0, -1, None, 0, None)),        # no dictionary
                     (lib.fsm_hip_keys_find_device, (None, p, None, 0, 0, 256, None, 0, None)),
                     (lib.fsm_hip_keys_find_device, (None, p, None, 0, 0, -1, None, 2, None)),
                     (lib.fsm_hip_keys_find_device, (None, p, None, 2 ** 32 - 1, 0, -1, None, 0, None)),      # (EOVERFLOW comes behind both)
                     (lib.fsm_hip_keys_find, (None, None, None, 1, -1, None, 0)),
                     (lib.fsm_hip_keys_find, (None, p, None, 1, -2, None, 0)),
                     (lib.fsm_hip_keys_find, (None, d, abc, 2, -1, None, 0)),
                     (lib.fsm_hip_keys_find, (None, p, None, 2 ** 40, -1, None, 0)),
                     (lib.fsm_hip_keys_find_extracted, (None, None, 0, None)),
                     (lib.fsm_hip_keys_find_hits, (None, None, 0, None)),
                     (lib.fsm_hip_keys_find_text, (None, None, 0, None))):
        C.set_errno(0)
        assert not fn(*args) and C.get_errno() == (errno.EINVAL if have else errno.ENODEV), (fn, args)
    # the getters of no object
    assert lib.fsm_hip_found_records(None) == 0 and lib.fsm_hip_found_present(None) == 0
    assert not lib.fsm_hip_found_class_device(None) and not lib.fsm_hip_found_bitmap_device(None) and not lib.fsm_hip_found_pick_device(None)
    for fn, args in ((lib.fsm_hip_found_copy, (None, None, None, None)), (lib.fsm_hip_found_ms, (None,)), (lib.fsm_hip_found_pass_ms, (None, 0))):
        C.set_errno(0)
        assert fn(*args) == -1 and C.get_errno() == errno.EINVAL
    lib.fsm_hip_found_free(None)


class _Stub:
    """stands in for the loaded library: every attribute is a function that records (name, arguments)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name,) + args)


def _made(cls, handle=0x1000, keep=("kept",)):
    obj = cls.__new__(cls)
    obj._lib, obj._h, obj._keep = _Stub(), handle, keep
    return obj


def test_the_object_owns_its_handle_as_the_other_objects_do():
    """the rules that hold every owner, held here for HipFound: the free function is in the table, close() frees exactly once,
    free() and the finaliser reach the same close(), also an overridden one, and a half-constructed object frees nothing"""
    import gc
    from libfsm_amd import capi
    cls = capi.HipFound
    assert capi.PROTOTYPES[cls._FREE] == (None, [C.c_void_p]) and cls._FREE == "fsm_hip_found_free"
    assert cls.close is capi._Owned.close and cls.free is capi._Freed.free and cls.handle is capi._Owned.handle
    obj = _made(cls)
    lib = obj._lib
    assert obj.handle == 0x1000
    obj.close()
    assert lib.calls == [(cls._FREE, 0x1000)] and obj._h is None and obj._keep is None and obj.handle is None
    obj.close()
    obj.free()
    obj.__del__()
    assert lib.calls == [(cls._FREE, 0x1000)]
    obj = _made(cls)
    obj.free()
    assert obj._lib.calls == [(cls._FREE, 0x1000)] and obj._h is None

    class Loud(cls):
        closed = 0

        def close(self):
            Loud.closed += 1
            super().close()

    obj = _made(Loud)
    obj.free()
    assert Loud.closed == 1 and obj._lib.calls == [(cls._FREE, 0x1000)]
    del obj                                          # (its finaliser closes once more, and frees nothing)
    gc.collect()
    obj, before = _made(Loud), Loud.closed
    lib = obj._lib
    del obj
    gc.collect()
    assert Loud.closed == before + 1 and lib.calls == [(cls._FREE, 0x1000)]
    # __init__ raised before there was a handle: no _h, no _keep, perhaps no _lib
    obj = cls.__new__(cls)
    obj.close()
    obj.__del__()
    obj = _made(cls, handle=None)
    obj.close()
    assert obj._lib.calls == []
