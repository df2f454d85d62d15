"""CPU: the distinct records (include/fsm_hip.h, "distinct").  The judge of tests/distinct_ref.py on cases by hand, and the entry
points: declared, exported, in the binding's table, failing LOUDLY without a device; the table size, which needs none."""
import ctypes as C
import errno

import numpy as np
import pytest

import distinct_ref

SYMBOLS = ("fsm_hip_distinct_device", "fsm_hip_distinct", "fsm_hip_extracted_distinct", "fsm_hip_text_hits_distinct", "fsm_hip_distinct_count",
           "fsm_hip_distinct_records", "fsm_hip_distinct_nbytes", "fsm_hip_distinct_first_device", "fsm_hip_distinct_count_device",
           "fsm_hip_distinct_class_device", "fsm_hip_distinct_off_device", "fsm_hip_distinct_bytes_device", "fsm_hip_distinct_copy",
           "fsm_hip_distinct_ms", "fsm_hip_distinct_pass_ms", "fsm_hip_distinct_free", "fsm_hip_distinct_long_bytes",
           "fsm_hip_distinct_table_slots")


def test_judge_on_cases_by_hand():
    off, data = distinct_ref.pack([b"a\n", b"b\n", b"a", b"\n", b"", b"b\n\n", b"ab", b"abc"])
    first, count, cls, doff, dbytes = distinct_ref.distinct(off, data, trim=0x0A, sep=0x0A)
    assert first.tolist() == [0, 1, 3, 5, 6, 7] and count.tolist() == [2, 1, 2, 1, 1, 1] and cls.tolist() == [0, 1, 0, 2, 2, 3, 4, 5]
    assert bytes(dbytes) == b"a\nb\n\nb\n\nab\nabc\n" and doff.tolist() == [0, 2, 4, 5, 8, 11, 15]
    # no trim: every record is itself; no separator: the keys back to back
    first, count, cls, doff, dbytes = distinct_ref.distinct(off, data)
    assert len(first) == 8 and (count == 1).all() and bytes(dbytes) == bytes(data) and np.array_equal(doff, off)
    # tags: equal bytes under different tags are different keys
    first, count, cls, _, dbytes = distinct_ref.distinct(*distinct_ref.pack([b"x", b"x", b"x", b"y"]), tag=[1, 2, 1, 2], sep=ord(","))
    assert first.tolist() == [0, 1, 3] and count.tolist() == [2, 1, 1] and cls.tolist() == [0, 1, 0, 2] and bytes(dbytes) == b"x,x,y,"
    # offsets are clamped to the bytes that may be read and to their predecessor
    first, count, cls, doff, dbytes = distinct_ref.distinct([0, 2, 1, 9], b"abcd", nbytes=3)
    assert distinct_ref.keys_of([0, 2, 1, 9], b"abcd", nbytes=3) == [b"ab", b"", b"bc"] and len(first) == 3
    # no record
    first, count, cls, doff, dbytes = distinct_ref.distinct([0], b"")
    assert len(first) == len(count) == len(cls) == len(dbytes) == 0 and doff.tolist() == [0]
    assert distinct_ref.table_slots(0) == distinct_ref.table_slots(8) == 16 and distinct_ref.table_slots(9) == 32


def test_every_new_symbol_is_declared_exported_and_in_the_table(built):
    import libfsm_amd
    from libfsm_amd import capi
    from test_abi import declared_symbols
    lib = libfsm_amd.load_library()
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert [s for s in SYMBOLS if s not in capi.PROTOTYPES] == []
    assert [s for s in SYMBOLS if s not in declared_symbols()] == []
    assert sorted(s for s in declared_symbols() if "distinct" in s) == sorted(SYMBOLS)
    assert libfsm_amd.DISTINCT_NO_TEXT == distinct_ref.NO_TEXT == 1 and libfsm_amd.DISTINCT_WEAK_HASH == distinct_ref.WEAK_HASH == 2
    for name in ("count", "records", "nbytes", "first_ptr", "count_ptr", "class_ptr", "off_ptr", "bytes_ptr", "copy", "ms", "pass_ms", "free"):
        assert hasattr(libfsm_amd.HipDistinct, name), name
    assert callable(libfsm_amd.HipExtracted.distinct) and callable(libfsm_amd.HipHits.distinct)
    assert callable(libfsm_amd.distinct_device) and callable(libfsm_amd.distinct)


def test_the_sizes_need_no_device(built):
    import libfsm_amd
    assert 16 <= libfsm_amd.distinct_long_bytes() <= 4096 and libfsm_amd.distinct_long_bytes() % 16 == 0
    for R in (0, 1, 7, 8, 9, 15, 16, 17, 300, 1000, 65535, 65536, 65537, 10 ** 6, 2 ** 31, distinct_ref.MAX_RECORDS):
        s = libfsm_amd.distinct_table_slots(R)
        assert s >= 16 and s >= 2 * R and s & (s - 1) == 0 and s == distinct_ref.table_slots(R), R
    for R in (distinct_ref.MAX_RECORDS + 1, 2 ** 40):
        with pytest.raises(OSError) as ei:
            libfsm_amd.distinct_table_slots(R)
        assert ei.value.errno == errno.EOVERFLOW


def test_no_distinct_without_a_device(built):
    """no CPU path: ENODEV from every entry point before any argument check (with a device, these arguments are EINVAL)"""
    import torch
    import libfsm_amd
    want = errno.EINVAL if torch.cuda.is_available() else errno.ENODEV
    lib = libfsm_amd.load_library()
    off = np.zeros(2, np.uint64)
    p = off.ctypes.data_as(C.c_void_p)
    for fn, args in ((lib.fsm_hip_distinct_device, (None, None, 1, 0, -1, None, -1, 0, None)),
                     (lib.fsm_hip_distinct_device, (p, None, 0, 0, 256, None, -1, 0, None)),
                     (lib.fsm_hip_distinct_device, (p, None, 0, 0, -1, None, -1, 4, None)),
                     (lib.fsm_hip_distinct, (None, None, 1, -1, None, -1, 0)),
                     (lib.fsm_hip_distinct, (p, None, 1, -1, None, -2, 0)),
                     (lib.fsm_hip_extracted_distinct, (None, -1, 0, None)),
                     (lib.fsm_hip_text_hits_distinct, (None, -1, 0, None))):
        C.set_errno(0)
        assert not fn(*args) and C.get_errno() == want, fn
    if not torch.cuda.is_available():
        # ... and before EOVERFLOW
        C.set_errno(0)
        assert not lib.fsm_hip_distinct_device(p, None, 2 ** 32, 0, -1, None, -1, 0, None) and C.get_errno() == errno.ENODEV
        with pytest.raises(OSError) as ei:
            libfsm_amd.distinct([0, 1], b"a")
        assert ei.value.errno == errno.ENODEV
    # the getters of no object
    assert lib.fsm_hip_distinct_count(None) == 0 and lib.fsm_hip_distinct_records(None) == 0 and lib.fsm_hip_distinct_nbytes(None) == 0
    assert not lib.fsm_hip_distinct_first_device(None) and not lib.fsm_hip_distinct_off_device(None)
    C.set_errno(0)
    assert lib.fsm_hip_distinct_copy(None, None, None, None, None, None) == -1 and C.get_errno() == errno.EINVAL
    lib.fsm_hip_distinct_free(None)


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
    """HipDistinct does not derive from the binding's owner class, so the rules that hold every owner are held here: the free
    function is in the table, close() frees exactly once, free() and the finaliser reach the same close(), also an overridden
    one, and a half-constructed object frees nothing"""
    import gc
    from libfsm_amd import capi
    cls = capi.HipDistinct
    assert capi.PROTOTYPES[cls._FREE] == (None, [C.c_void_p]) and cls._FREE == "fsm_hip_distinct_free"
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
