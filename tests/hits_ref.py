"""Test helper of the text front's hits (tests/test_gpu_text_hits.py, tests/tools/hits_probe.py): the selection rule of
include/fsm_hip.h ("The hits") stated once in numpy, independent of the code under test."""
import numpy as np

from text_ref import split_ref


def hits_ref(text, delim, bits, invert=False):
    """(lines, out_off, out) for a text, its delimiter and one bool per line (bits beyond the n lines are ignored):
    the selected lines' indices, the m + 1 output offsets and the selected lines' bytes, trailing delimiters included."""
    text = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text, np.uint8)
    off = split_ref(text, delim)
    n = len(off) - 1
    sel = np.asarray(bits, bool)[:n] ^ bool(invert)
    lines = np.flatnonzero(sel).astype(np.uint64)
    lens = np.diff(off.astype(np.int64))
    out = text[np.repeat(sel, lens)]
    out_off = np.concatenate([[0], np.cumsum(lens[sel])]).astype(np.uint64)
    return lines, out_off, out


def pack_bits(bits, garbage=0):
    """the bitmap of ceil(n / 64) words, bit i = line i; the bits at and above n of the last word all `garbage` (0 or 1)"""
    bits = np.asarray(bits, bool)
    n = len(bits)
    full = np.full((n + 63) // 64 * 64, bool(garbage))
    full[:n] = bits
    return np.packbits(full, bitorder="little").view(np.uint64) if n else np.zeros(0, np.uint64)
