"""CPU: the extraction (include/fsm_hip.h, "extract").  The judge of tests/extract_ref.py against Python's re.finditer on the
keyword pair of test_matches_abi.word_lines() -- every rule kept with a newline, a kept subset, empty matches without a
separator -- and the entry points: exported, in the binding's table, failing LOUDLY without a device."""
import ctypes as C
import errno
import os
import re

import numpy as np
import pytest

import extract_ref
import matches_ref
import span_ref
import tokens_ref
from span_ref import rows_of
from test_matches_abi import WORDS, word_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("fsm_hip_rules_create", "fsm_hip_rules_free", "fsm_hip_matches_extract", "fsm_hip_matches_extract_device", "fsm_hip_text_extract",
           "fsm_hip_extracted_count", "fsm_hip_extracted_nbytes", "fsm_hip_extracted_off_device", "fsm_hip_extracted_bytes_device",
           "fsm_hip_extracted_line_device", "fsm_hip_extracted_match_device", "fsm_hip_extracted_copy", "fsm_hip_extracted_ms",
           "fsm_hip_extracted_pass_ms", "fsm_hip_extracted_free", "fsm_hip_extracted_block_matches", "fsm_hip_extracted_block_bytes")
# the alternation ordered longest-first: leftmost-longest for literals
PATTERN = re.compile(b"|".join(re.escape(w) for w in sorted(WORDS, key=len, reverse=True)))


def keyword_matches(lines):
    """(rows, lens, (off, start, end, id)) of the keywords' pair, the id of a match the index of its word"""
    rows, lens = rows_of(lines)
    ends, sets = tokens_ref.trie_lexer(WORDS)
    ids = tokens_ref.state_ids(ends, tokens_ref.EARLIEST, sets)
    res = matches_ref.matches(span_ref.starts_of(WORDS), ends, rows, lens, ids=ids)
    return rows, lens, (res["off"], res["start"], res["end"], res["id"])


def test_judge_is_re_finditer_on_the_keywords():
    lines = word_lines()
    rows, lens, mt = keyword_matches(lines)
    assert len(mt[1]) >= 5000 and set(mt[3].tolist()) == set(range(len(WORDS)))
    # every rule kept, with a newline: what grep -o prints
    off, data, line, match = extract_ref.extract(rows, lens, lens, mt, sep=0x0A)
    found = [(i, mo) for i, x in enumerate(lines) for mo in PATTERN.finditer(x)]
    assert bytes(data) == b"".join(mo.group() + b"\n" for _, mo in found)
    assert line.tolist() == [i for i, _ in found] and match.tolist() == list(range(len(mt[1])))
    assert extract_ref.records_of(off, data) == [mo.group() + b"\n" for _, mo in found]
    assert [int(mt[1][k]) for k in match] == [mo.start() for _, mo in found]
    # no set and a set of every rule are the same; so is an empty set with KEEP_OTHER and nrules = 0
    for keep, other in (((len(WORDS), set(range(len(WORDS)))), False), ((0, set()), True)):
        again = extract_ref.extract(rows, lens, lens, mt, keep, other, 0x0A)
        assert all(np.array_equal(a, b) for a, b in zip(again, (off, data, line, match)))
    # a kept subset: the same, filtered by word; without a separator the records are the words themselves
    for kept, other in (({0, 3}, False), ({1}, False), (set(), False), ({2, 4}, True)):
        words = {WORDS[i] for i in kept}
        want = [(i, mo) for i, mo in found if mo.group() in words]
        off, data, line, match = extract_ref.extract(rows, lens, lens, mt, (len(WORDS), kept), other, 0x0A)
        assert bytes(data) == b"".join(mo.group() + b"\n" for _, mo in want)
        assert line.tolist() == [i for i, _ in want] and len(off) == len(want) + 1
        assert all(WORDS[int(mt[3][k])] in words for k in match)
        off, data, _, _ = extract_ref.extract(rows, lens, lens, mt, (len(WORDS), kept), other, -1)
        assert extract_ref.records_of(off, data) == [mo.group() for _, mo in want]
    # a set of the first two rules alone: the other three are "beyond the set" and come in with KEEP_OTHER only
    off, data, _, _ = extract_ref.extract(rows, lens, lens, mt, (2, {1}), False, 0x0A)
    assert bytes(data) == b"".join(mo.group() + b"\n" for _, mo in found if mo.group() == WORDS[1])
    off, data, _, _ = extract_ref.extract(rows, lens, lens, mt, (2, {1}), True, 0x0A)
    assert bytes(data) == b"".join(mo.group() + b"\n" for _, mo in found if mo.group() != WORDS[0])


def test_judge_keeps_empty_matches_as_empty_records():
    """x* with every position a start: without a separator the empty matches are records without bytes and off repeats"""
    lines = [b"", b"x", b"abxd", b"xxaxx", b"abc"] + [bytes(np.frombuffer(b"axb", np.uint8)[np.random.RandomState(31).randint(0, 3, k)]) for k in range(40)]
    rows, lens = rows_of(lines)
    dense = np.full((1, 256), -1, np.int64)
    dense[0, ord("x")] = 0
    ends = span_ref._auto(dense, [True])
    starts = span_ref.everywhere_of(span_ref.starts_of([b"x"]))
    res = matches_ref.matches(starts, ends, rows, lens, ids=np.zeros(1, np.int64))
    mt = (res["off"], res["start"], res["end"], res["id"])
    found = [(i, mo) for i, x in enumerate(lines) for mo in re.finditer(b"x*", x)]
    off, data, line, match = extract_ref.extract(rows, lens, lens, mt)
    assert extract_ref.records_of(off, data) == [mo.group() for _, mo in found]
    assert line.tolist() == [i for i, _ in found]
    empty = np.diff(off.astype(np.int64)) == 0
    assert empty.sum() >= 100 and (~empty).sum() >= 50 and set(bytes(data)) == {ord("x")}
    assert extract_ref.records_of(off, data)[:4] == [b"", b"x", b"", b""]          # "", then "x": x and the empty match behind it
    # with a separator every record has a byte: the empty ones are the separator alone
    off, data, _, _ = extract_ref.extract(rows, lens, lens, mt, sep=0)
    assert extract_ref.records_of(off, data) == [mo.group() + b"\0" for _, mo in found]
    # every match is clamped on its own: one that leaves the line is cut, one behind it is empty, start > end is empty at end
    text = np.frombuffer(b"abcdef", np.uint8)[None, :]
    wild = (np.array([0, 4], np.uint64), np.array([2, 9, 5, 0], np.uint64), np.array([9, 12, 3, 2 ** 64 - 1], np.uint64), np.zeros(4, np.uint32))
    off, data, _, _ = extract_ref.extract(text, [6], [6], wild, sep=ord("|"))
    assert bytes(data) == b"cdef|||abcdef|"


def test_every_new_symbol_is_exported_and_in_the_table(built):
    import libfsm_amd
    from libfsm_amd import capi
    lib = libfsm_amd.load_library()
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert [s for s in SYMBOLS if s not in capi.PROTOTYPES] == []
    header = open(os.path.join(ROOT, "include", "fsm_hip.h")).read()
    assert [s for s in SYMBOLS if s + "(" not in header] == []
    assert libfsm_amd.RULES_KEEP_OTHER == extract_ref.KEEP_OTHER == 1
    for name in ("HipRules", "HipExtracted"):
        assert hasattr(libfsm_amd, name)
    for name in ("extract", "extract_device", "text_extract"):
        assert callable(getattr(libfsm_amd.HipMatches, name))
    # the constants need no device
    assert libfsm_amd.extracted_block_matches() == 256 and libfsm_amd.extracted_block_bytes() == 16384


def test_no_extraction_without_a_device(built):
    """no CPU path: ENODEV from every entry point that would launch or upload, whatever the arguments (with a device, these
    arguments are EINVAL)"""
    import torch
    import libfsm_amd
    want = errno.EINVAL if torch.cuda.is_available() else errno.ENODEV
    lib = libfsm_amd.load_library()
    b = libfsm_amd.MatchBatch()
    for fn, args in ((lib.fsm_hip_rules_create, (None, 1, 0)), (lib.fsm_hip_rules_create, (None, 0, 2)),
                     (lib.fsm_hip_matches_extract, (None, C.byref(b), None, -1)), (lib.fsm_hip_matches_extract, (None, None, None, 300)),
                     (lib.fsm_hip_matches_extract_device, (None, C.byref(b), None, -1, None)),
                     (lib.fsm_hip_text_extract, (None, None, None, None, -1, None))):
        C.set_errno(0)
        assert fn(*args) is None and C.get_errno() == want
    if not torch.cuda.is_available():
        with pytest.raises(OSError) as ei:
            libfsm_amd.HipRules([0], 1)
        assert ei.value.errno == errno.ENODEV


def test_accessors_take_null(built):
    import libfsm_amd
    lib = libfsm_amd.load_library()
    out = np.zeros(2, np.uint64)
    assert lib.fsm_hip_extracted_count(None) == 0 and lib.fsm_hip_extracted_nbytes(None) == 0
    for fn in (lib.fsm_hip_extracted_off_device, lib.fsm_hip_extracted_bytes_device, lib.fsm_hip_extracted_line_device,
               lib.fsm_hip_extracted_match_device):
        assert fn(None) is None
    C.set_errno(0)
    assert lib.fsm_hip_extracted_copy(None, out.ctypes.data_as(C.c_void_p), None, None, None) == -1 and C.get_errno() == errno.EINVAL
    C.set_errno(0)
    assert lib.fsm_hip_extracted_ms(None) == -1.0 and C.get_errno() == errno.EINVAL
    C.set_errno(0)
    assert lib.fsm_hip_extracted_pass_ms(None, 0) == -1.0 and C.get_errno() == errno.EINVAL
    lib.fsm_hip_extracted_free(None)     # as free(NULL)
    lib.fsm_hip_rules_free(None)
