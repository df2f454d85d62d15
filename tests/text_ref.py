"""Test helpers of the text front (tests/test_text_desc.py, tests/test_gpu_text.py, tests/tools/text_probe.py): the line rule
stated once in numpy, independent of the code under test, and the oracle's answers line by line."""
import numpy as np

from libfsm_amd import FlatDfa, NO_MATCH


def split_ref(buf, delim):
    """The n + 1 offsets of the lines of buf (include/fsm_hip.h, "text front"): every delimiter ends a line; bytes after the
    last delimiter form a last line iff there are any; an empty text has 0 lines; two delimiters in a row enclose an empty
    line.  off[0] = 0, off[k] = position of the k-th delimiter + 1, off[n] = len(buf)."""
    buf = np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray)) else np.asarray(buf, np.uint8)
    ends = np.flatnonzero(buf == np.uint8(delim)).astype(np.uint64) + np.uint64(1)
    off = np.concatenate([np.zeros(1, np.uint64), ends])
    if len(buf) and buf[-1] != delim:
        off = np.concatenate([off, np.array([len(buf)], np.uint64)])
    return off


def squeeze_ref(buf, delim):
    """What examples/hipgrep.c hands the library: the text with its delimiters squeezed out, and the lines' offsets in it."""
    buf = np.asarray(buf, np.uint8)
    off = split_ref(buf, delim)
    n = len(off) - 1
    ndel = np.cumsum(buf == np.uint8(delim))          # delimiters up to and including position p
    before = np.concatenate([np.zeros(1, np.int64), ndel])[off.astype(np.int64)]   # delimiters before position off[k]
    return buf[buf != np.uint8(delim)], (off.astype(np.int64) - before).astype(np.uint64), n


def newline_dfa():
    """a\\nb | a+ : an automaton whose ORIGINAL has a real transition on '\\n' (state 1 -'\\n'-> 2), with end-ids and eager
    outputs, so that a transform which only fills missing edges keeps the edge and fails.  Without its newlines "a\\nb" is
    "ab", which the original rejects (1 -b-> nothing) and "aa" is accepted in state 1."""
    nt = np.full((4, 256), -1, np.int64)
    nt[0, ord("a")] = 1
    nt[1, ord("a")] = 1
    nt[1, 0x0A] = 2
    nt[2, ord("b")] = 3
    nt[2, 0x0A] = 0
    eager_off = np.array([0, 1, 2, 3, 5], np.uint32)
    eager_ids = np.array([7, 11, 13, 7, 17], np.uint32)
    return FlatDfa.from_dense(nt, 0, [0, 1, 0, 1], endids={1: [4, 2], 3: [9]}, eager_off=eager_off, eager_ids=eager_ids)


def rows_of(strings):
    """fixed-stride rows + lengths of a list of byte strings (the oracle's eager walk takes rows)"""
    stride = max([len(s) for s in strings] + [1])
    rows = np.zeros((len(strings), stride), np.uint8)
    for i, s in enumerate(strings):
        rows[i, :len(s)] = np.frombuffer(s, np.uint8)
    return rows, np.array([len(s) for s in strings], np.uint32)


def oracle_answers(flat, strings):
    """(ret, end with NO_MATCH for rejects, end-id tuple per input, eager id set per input) by the oracle over `flat`"""
    from oracle.pyoracle import Oracle
    o = Oracle(flat)
    rows, lens = rows_of(strings)
    ret, end, sets = o.exec_eager(rows, lens, cap=256)
    end = np.where(ret == 1, end, NO_MATCH).astype(np.uint32)
    ids = [tuple(int(x) for x in o.endids(int(e))) if r == 1 else None for r, e in zip(ret, end)]
    return ret, end, ids, [frozenset(int(x) for x in s) for s in sets]


def lines_of(buf, delim):
    """the lines WITHOUT their delimiters, by bytes.split: the piece after the last delimiter is a line iff it has bytes"""
    parts = bytes(np.asarray(buf, np.uint8)).split(bytes([delim]))
    return parts[:-1] if parts[-1] == b"" else parts
