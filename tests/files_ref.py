"""Test helper of the text front's files (tests/test_text_files_abi.py, tests/test_gpu_text_files.py, tests/tools/files_probe.py):
the rule of include/fsm_hip.h ("Files of a text") stated in numpy, independent of the code under test, and a hits reference
that takes given offsets (hits_ref.hits_ref cuts the text itself)."""
import numpy as np

from text_ref import split_ref


def as_u8(buf):
    return np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray)) else np.asarray(buf, np.uint8)


def files_ref(buf, delim, file_off):
    """(off, file_lines): the sorted union without duplicates of the plain offsets and the file ends; the index of every file end in it"""
    file_off = np.asarray(file_off, np.uint64)
    off = np.unique(np.concatenate([split_ref(as_u8(buf), delim), file_off]))
    return off, np.searchsorted(off, file_off).astype(np.uint64)


def files_ref_each(buf, delim, file_off):
    """the second statement of the rule: every file cut alone by split_ref, shifted to its place, in file order"""
    buf = as_u8(buf)
    fo = [int(x) for x in file_off]
    off, file_lines = [np.zeros(1, np.uint64)], [0]
    n = 0
    for a, b in zip(fo[:-1], fo[1:]):
        o = split_ref(buf[a:b], delim)
        off.append(o[1:] + np.uint64(a))
        n += len(o) - 1
        file_lines.append(n)
    return np.concatenate(off), np.array(file_lines, np.uint64)


def hits_ref_off(text, off, bits, invert=False):
    """hits_ref over GIVEN offsets: (lines, out_off, out) of the lines [off[i], off[i + 1]) that bits (^ invert) select"""
    text = as_u8(text)
    n = len(off) - 1
    sel = np.asarray(bits, bool)[:n] ^ bool(invert)
    lines = np.flatnonzero(sel).astype(np.uint64)
    lens = np.diff(np.asarray(off).astype(np.int64))
    out = text[np.repeat(sel, lens)]
    out_off = np.concatenate([[0], np.cumsum(lens[sel])]).astype(np.uint64)
    return lines, out_off, out


def join_files(files):
    """the files back to back with nothing between them, and their file_off"""
    return np.frombuffer(b"".join(files), np.uint8), np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.uint64)
