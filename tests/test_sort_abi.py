"""CPU: the sort of a packed text (include/fsm_hip.h, "sort").  The judge of tests/sort_ref.py on cases by hand, and the entry
points: declared, exported, in the binding's table, failing LOUDLY without a device -- ENODEV before any argument check; with a
device the same arguments are refused for what they are."""
import ctypes as C
import errno

import numpy as np
import pytest

import sort_ref
from distinct_ref import pack

SYMBOLS = ("fsm_hip_sort_device", "fsm_hip_sort", "fsm_hip_extracted_sort", "fsm_hip_text_hits_sort", "fsm_hip_keys_sort", "fsm_hip_sorted_records",
           "fsm_hip_sorted_groups", "fsm_hip_sorted_nbytes", "fsm_hip_sorted_rounds", "fsm_hip_sorted_radix_passes", "fsm_hip_sorted_order_device",
           "fsm_hip_sorted_rank_device", "fsm_hip_sorted_off_device", "fsm_hip_sorted_bytes_device", "fsm_hip_sorted_copy", "fsm_hip_sorted_ms",
           "fsm_hip_sorted_pass_ms", "fsm_hip_sort_tile_records", "fsm_hip_sorted_free")


def test_judge_on_cases_by_hand():
    recs = [b"b\n", b"a", b"", b"ab\n", b"a\n", b"\x00", b"\n", b"\x00\x00", b"\xff", b"ab\x00"]
    off, data = pack(recs)
    order, rank, groups, soff, sbytes = sort_ref.sort(off, data, trim=0x0A, sep=0x0A)
    assert order.tolist() == [2, 6, 5, 7, 1, 4, 3, 9, 0, 8] and rank.tolist() == [0, 0, 1, 2, 3, 3, 4, 5, 6, 7] and groups == 8
    assert bytes(sbytes) == b"\n\n\x00\n\x00\x00\na\na\nab\nab\x00\nb\n\xff\n" and soff.tolist() == [0, 1, 2, 4, 7, 9, 11, 14, 18, 20, 22]
    # REVERSE: the longer key before its prefix, ties still ascending in r
    order, rank, groups, _, sbytes = sort_ref.sort(off, data, trim=0x0A, flags=sort_ref.REVERSE)
    assert order.tolist() == [8, 0, 9, 3, 1, 4, 7, 5, 2, 6] and rank.tolist() == [0, 1, 2, 3, 4, 4, 5, 6, 7, 7] and bytes(sbytes) == b"\xffbab\x00abaa\x00\x00\x00"
    # major first, the key second; equal (major, key) pairs are one group
    recs = [b"x", b"a", b"x", b"a", b"m"]
    major = [2, 2 ** 64 - 1, 2, 0, 2]
    order, rank, groups, _, _ = sort_ref.sort(*pack(recs), major=major)
    assert order.tolist() == [3, 4, 0, 2, 1] and rank.tolist() == [0, 1, 2, 2, 3] and groups == 4
    order, rank, _, _, _ = sort_ref.sort(*pack(recs), major=major, flags=sort_ref.MAJOR_DESC)
    assert order.tolist() == [1, 4, 0, 2, 3] and rank.tolist() == [0, 1, 2, 2, 3]
    order, _, _, _, _ = sort_ref.sort(*pack(recs), major=major, flags=sort_ref.MAJOR_DESC | sort_ref.REVERSE)
    assert order.tolist() == [1, 0, 2, 4, 3]
    # offsets are clamped as the distinct records clamp them; no record
    order, _, groups, soff, sbytes = sort_ref.sort([0, 2, 1, 9], b"abcd", nbytes=3, sep=ord(","))
    assert order.tolist() == [1, 0, 2] and bytes(sbytes) == b",ab,bc," and groups == 3
    order, rank, groups, soff, sbytes = sort_ref.sort([0], b"")
    assert len(order) == len(rank) == len(sbytes) == 0 and soff.tolist() == [0] and groups == 0


def test_every_new_symbol_is_declared_exported_and_in_the_table(built):
    import libfsm_amd
    from libfsm_amd import capi
    from test_abi import declared_symbols
    lib = libfsm_amd.load_library()
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert [s for s in SYMBOLS if s not in capi.PROTOTYPES] == []
    assert sorted(s for s in declared_symbols() if "sort" in s) == sorted(SYMBOLS)
    assert (libfsm_amd.SORT_NO_TEXT, libfsm_amd.SORT_REVERSE, libfsm_amd.SORT_MAJOR_DESC, libfsm_amd.SORT_BY_COUNT) == (1, 2, 4, 8)
    assert (sort_ref.NO_TEXT, sort_ref.REVERSE, sort_ref.MAJOR_DESC, sort_ref.BY_COUNT) == (1, 2, 4, 8)
    for name in ("records", "groups", "nbytes", "rounds", "radix_passes", "order_ptr", "rank_ptr", "off_ptr", "bytes_ptr", "copy", "ms", "pass_ms", "free"):
        assert hasattr(libfsm_amd.HipSorted, name), name
    assert callable(libfsm_amd.HipExtracted.sort) and callable(libfsm_amd.HipHits.sort) and callable(libfsm_amd.HipDistinct.sort)
    assert callable(libfsm_amd.sort_device) and callable(libfsm_amd.sort)
    cls = capi.HipSorted
    assert capi.PROTOTYPES[cls._FREE] == (None, [C.c_void_p]) and cls.close is capi._Owned.close and cls.free is capi._Freed.free


def test_the_tile_needs_no_device(built):
    import libfsm_amd
    t = libfsm_amd.sort_tile_records()
    assert 256 <= t <= 65536 and t % 256 == 0


def test_no_sort_without_a_device(built):
    """no CPU path: ENODEV from every entry point before any argument check; with a device each argument is refused for itself"""
    import torch
    import libfsm_amd
    have = torch.cuda.is_available()
    lib = libfsm_amd.load_library()
    off = np.zeros(2, np.uint64)
    down = np.array([0, 3, 2], np.uint64)
    mj = np.zeros(2, np.uint64)
    p, d, m = (a.ctypes.data_as(C.c_void_p) for a in (off, down, mj))
    abc = C.c_char_p(b"abc")
    for fn, args, with_device in (
            (lib.fsm_hip_sort_device, (None, None, 1, 0, -1, None, -1, 0, None), errno.EINVAL),         # d_off NULL
            (lib.fsm_hip_sort_device, (p, None, 0, 0, 256, None, -1, 0, None), errno.EINVAL),           # trim_byte
            (lib.fsm_hip_sort_device, (p, None, 0, 0, -2, None, -1, 0, None), errno.EINVAL),
            (lib.fsm_hip_sort_device, (p, None, 0, 0, -1, None, 256, 0, None), errno.EINVAL),           # sep_byte
            (lib.fsm_hip_sort_device, (p, None, 0, 0, -1, None, -1, 16, None), errno.EINVAL),           # an unknown flag
            (lib.fsm_hip_sort_device, (p, None, 0, 0, -1, None, -1, 0x80000000, None), errno.EINVAL),
            (lib.fsm_hip_sort_device, (p, None, 0, 0, -1, None, -1, sort_ref.MAJOR_DESC, None), errno.EINVAL),   # MAJOR_DESC without major
            (lib.fsm_hip_sort_device, (p, None, 0, 0, -1, m, -1, sort_ref.BY_COUNT, None), errno.EINVAL),        # BY_COUNT is the keys' alone
            (lib.fsm_hip_sort_device, (p, None, 2 ** 32 - 1, 0, -1, None, -1, 0, None), errno.EOVERFLOW),
            (lib.fsm_hip_sort, (None, None, 1, -1, None, -1, 0), errno.EINVAL),
            (lib.fsm_hip_sort, (p, None, 1, -1, None, -2, 0), errno.EINVAL),
            (lib.fsm_hip_sort, (p, None, 1, -1, None, -1, sort_ref.MAJOR_DESC), errno.EINVAL),
            (lib.fsm_hip_sort, (p, None, 1, -1, m, -1, sort_ref.BY_COUNT), errno.EINVAL),
            (lib.fsm_hip_sort, (d, abc, 2, -1, None, -1, 0), errno.EINVAL),                              # decreasing offsets
            (lib.fsm_hip_extracted_sort, (None, -1, 0, None), errno.EINVAL),
            (lib.fsm_hip_text_hits_sort, (None, -1, 0, None), errno.EINVAL),
            (lib.fsm_hip_keys_sort, (None, -1, sort_ref.BY_COUNT, None), errno.EINVAL)):
        C.set_errno(0)
        assert not fn(*args) and C.get_errno() == (with_device if have else errno.ENODEV), (fn, args)
    if not have:
        with pytest.raises(OSError) as ei:
            libfsm_amd.sort([0, 1], b"a")
        assert ei.value.errno == errno.ENODEV
    # the getters of no object
    assert lib.fsm_hip_sorted_records(None) == 0 and lib.fsm_hip_sorted_groups(None) == 0 and lib.fsm_hip_sorted_nbytes(None) == 0
    assert lib.fsm_hip_sorted_rounds(None) == 0 and lib.fsm_hip_sorted_radix_passes(None, 0) == 0
    assert not lib.fsm_hip_sorted_order_device(None) and not lib.fsm_hip_sorted_rank_device(None)
    assert not lib.fsm_hip_sorted_off_device(None) and not lib.fsm_hip_sorted_bytes_device(None)
    for fn, args in ((lib.fsm_hip_sorted_copy, (None, None, None, None, None)), (lib.fsm_hip_sorted_ms, (None,)), (lib.fsm_hip_sorted_pass_ms, (None, 0))):
        C.set_errno(0)
        assert fn(*args) == -1 and C.get_errno() == errno.EINVAL
    lib.fsm_hip_sorted_free(None)
